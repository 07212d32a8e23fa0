"""The 12-wave form of the folded wave-resident frame-MLP kernel (frame_mlps_wr_kernel<false, true, 12>): 384
frames per workgroup and three waves per SIMD, for the audio half of a pipeline whose neighbouring batch's recurrence leaves
too few compute units for the 8-wave form's workgroups.  A wave's chain over its 32 frames is the same instructions on the same
values in either form, so every check against the 8-wave form is bit for bit.  GPU part (-m gpu): the two forms forced on the
same inputs at the block edges, which form the launcher picks for whom, one pipelined run end to end.  CPU part: the build's
register budget line for the instantiation."""
import ctypes as C
import importlib
import importlib.util
import os

import pytest
import torch

from conftest import ROOT

PKG = "neural-waveshaping-synthesis_amd"
CANARY = 12345.0


def _lib():
    return importlib.import_module(PKG + "._lib")


def _build():
    spec = importlib.util.spec_from_file_location("nws_build_waves", os.path.join(ROOT, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fast():
    from gpu_util import build_model

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return build_model(True)


def run_form(eng, gru, waves):
    """the folded kernel forced to `waves` waves per workgroup on gru (F, 128): film (F, 256), spectrum rows (F, 132) written into
    canary-filled buffers"""
    lib = _lib()
    F = gru.shape[0]
    film = torch.full((F, 256), CANARY, device="cuda")
    spec = torch.full((F, 132), CANARY, device="cuda")
    lib.check(lib.lib().nws_debug_frame_mlps_spec_waves(C.byref(eng.weights()[0]), lib.ptr(gru), F, lib.ptr(film), lib.ptr(spec),
                                                        waves, lib.stream_ptr()), "nws_debug_frame_mlps_spec_waves")
    torch.cuda.synchronize()
    return film, spec


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(1, 1), (1, 383), (1, 384), (1, 385), (1, 417), (3, 130)])
def test_twelve_waves_write_the_bits_of_eight(fast, B, T):
    """F = 1: eleven idle waves; 383 / 384 / 385: the block edge; 417: a second block of one full and one partial wave; 3 x 130 =
    390 frames: tiles that cross utterance boundaries (the kernel sees flattened frames).  FiLM rows and spectrum rows equal bit
    for bit, every row written, and the three floats behind bin 128 of a spectrum row left alone by both forms."""
    eng = fast._engine
    assert eng.weights()[0].mlp_spec == 1
    g = torch.Generator().manual_seed(1000 * B + T)
    gru = torch.tanh(torch.randn(B, T, 128, generator=g)).reshape(B * T, 128).cuda()
    film8, spec8 = run_form(eng, gru, 8)
    film12, spec12 = run_form(eng, gru, 12)
    assert _lib().lib().nws_debug_frame_mlps_last_waves() == 12
    assert torch.equal(film12, film8)
    assert torch.equal(spec12, spec8)
    assert bool((spec12[:, 129:] == CANARY).all()) and bool((spec8[:, 129:] == CANARY).all())
    assert bool((film12 != CANARY).all()) and bool((spec12[:, :129] != CANARY).all())
    assert bool(torch.isfinite(film12).all()) and bool(torch.isfinite(spec12[:, :129]).all())


@pytest.mark.gpu
def test_which_form_the_launcher_picks(fast):
    """nws_frame_mlps_spec_waves is the launcher's own rule: 12 waves where the audio half runs apart from its control half AND
    2 ceil(F / 256) > CUs - B >= 2 ceil(F / 384).  The forwards are asked what they launched (nws_debug_frame_mlps_last_waves)."""
    from gpu_util import build_model

    lib = _lib()
    L = lib.lib()
    eng = fast._engine
    w = eng.weights()[0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == 256, cus                                         # the arithmetic below is MI355X's
    assert L.nws_frame_mlps_spec_waves(C.byref(w), 64, 500, 1) == 12      # 250 > 192 >= 168
    assert L.nws_frame_mlps_spec_waves(C.byref(w), 64, 500, 0) == 8       # behind its own recurrence: the plain forward
    # B = 32: 32 x 500 is one frame short of the wave-resident kernel's threshold (32 x 8 tiles of 64 frames = 256, not more),
    # the tile kernels run and there is no folded launch to give a form to; from T = 513 on there is one, and its 130 workgroups
    # fit 224 compute units anyway
    assert L.nws_frame_mlps_spec_waves(C.byref(w), 32, 500, 1) == 0
    assert L.nws_frame_mlps_spec_waves(C.byref(w), 32, 520, 1) == 8
    assert L.nws_frame_mlps_spec_waves(C.byref(w), 64, 70, 1) == 0        # too few frames for the wave-resident kernel at all
    B, T = 64, 500
    g = torch.Generator().manual_seed(5)
    f0 = 100.0 + 600.0 * torch.rand(B, 1, T, generator=g).cuda()
    control = torch.randn(B, 2, T, generator=g).cuda()
    pu, nz = torch.rand(101, generator=g).cuda(), torch.rand(128 * T - 1, generator=g).cuda()
    with torch.no_grad():
        y = fast(f0, control, phase_u=pu, noise=nz)
        torch.cuda.synchronize()
        assert L.nws_debug_frame_mlps_last_waves() == 8            # nws_forward
        ws = eng.new_workspace(B, T)
        eng.forward_control(f0, control, ws, batched_gru=False)
        y2 = eng.forward_audio(f0, B, T, pu, nz, ws)
        torch.cuda.synchronize()
        assert L.nws_debug_frame_mlps_last_waves() == 12           # nws_forward_audio_ev
        assert torch.equal(y2, y)
        T32 = 520
        f32, c32 = 100.0 + 600.0 * torch.rand(32, 1, T32, generator=g).cuda(), torch.randn(32, 2, T32, generator=g).cuda()
        ws32 = eng.new_workspace(32, T32)
        eng.forward_control(f32, c32, ws32, batched_gru=False)
        eng.forward_audio(f32, 32, T32, pu, torch.rand(128 * T32 - 1, generator=g).cuda(), ws32)
        torch.cuda.synchronize()
        assert L.nws_debug_frame_mlps_last_waves() == 8            # the audio-half entry at B = 32
        # no folded tables (the range guard of tests/test_frame_spec.py refuses them): never the 12-wave form
        m = build_model(True)
        m.embedding.proj.weight.mul_(30.0)
        m.newt.mlp.net[0].weight.mul_(30.0)
        w0 = m._engine.weights()[0]
        assert w0.mlp_frags and w0.mlp_spec == 0
        assert L.nws_frame_mlps_spec_waves(C.byref(w0), 64, 500, 1) == 0
        ws0 = m._engine.new_workspace(B, T)
        m._engine.forward_control(f0, control, ws0, batched_gru=False)
        m._engine.forward_audio(f0, B, T, pu, nz, ws0)
        torch.cuda.synchronize()
        assert L.nws_debug_frame_mlps_last_waves() == 8            # still the 32-batch launch above: no folded launch since


@pytest.mark.gpu
def test_pipelined_run_equals_the_plain_forward(fast):
    """four batches of 64 x 500 through the default pipeline (its audio halves take the 12-wave form) against model() (8 waves)"""
    import nws_amd

    L = _lib().lib()
    B, T = 64, 500
    g = torch.Generator(device="cuda").manual_seed(9)
    jobs = []
    for _ in range(4):
        f0 = (100 + 900 * torch.rand(B, 1, 1, device="cuda", generator=g)) * (1 + 0.01 * torch.randn(B, 1, T, device="cuda", generator=g))
        jobs.append((f0, torch.randn(B, 2, T, device="cuda", generator=g), torch.rand(101, device="cuda", generator=g),
                     torch.rand(128 * T - 1, device="cuda", generator=g)))
    with torch.no_grad():
        refs = [fast(f0, c, phase_u=pu, noise=nz) for f0, c, pu, nz in jobs]
        torch.cuda.synchronize()
        assert L.nws_debug_frame_mlps_last_waves() == 8
        pipe = nws_amd.ForwardPipeline(fast)
        outs = [pipe.submit(f0, c, phase_u=pu, noise=nz) for f0, c, pu, nz in jobs]
        pipe.synchronize()
    assert L.nws_debug_frame_mlps_last_waves() == 12
    assert all(torch.equal(o, r) for o, r in zip(outs, refs))


REMARK = """x.hip:1:1: remark: Function Name: _ZN12_GLOBAL__N_120frame_mlps_wr_kernelILb0ELb1ELi12EEEv10NwsWeightsPKfiiPfS4_S4_S4_i [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     VGPRs: %d [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark: Function Name: _ZN12_GLOBAL__N_120frame_mlps_wr_kernelILb0ELb1ELi8EEEv10NwsWeightsPKfiiPfS4_S4_S4_i [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     VGPRs: 182 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
"""


def test_register_budget_line_of_the_twelve_wave_form():
    """three waves per SIMD are 512 / 3 registers in steps of 8 = 168: an invented remark of 176 for the instantiation fails the
    build rule, 168 passes, and the 8-wave instantiation beside it (182) is not the line's business.  Then the real translation
    unit: the line finds its kernel, which is inside it, and no kernel of the file uses scratch."""
    import subprocess

    b = _build()
    lines = [(key, budget) for key, budget, _ in b.REGISTER_BUDGETS_FRAME_MLPS]
    assert lines == [("frame_mlps_wr_kernelILb0ELb1ELi12E", 168)], lines
    over = b.check_register_budgets(REMARK % 176)
    assert [(n, bud) for _, n, bud, _ in over] == [(176, 168)] and "Li12E" in over[0][0], over
    assert b.check_register_budgets(REMARK % 168) == []
    src = "frame_mlps.hip"
    r = subprocess.run([b._hipcc(), *b.FLAGS, *b.EXTRA_FLAGS.get(src, []), "-c", os.path.join(b.CSRC, src), "-o", os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert b.check_register_budgets(r.stderr) == []
    regs = {k: n for k, n in b.kernel_registers(r.stderr).items() if "frame_mlps_wr_kernel" in k}
    twelve = [n for k, n in regs.items() if "frame_mlps_wr_kernelILb0ELb1ELi12E" in k]
    assert len(regs) == 4 and len(twelve) == 1 and 0 < twelve[0] <= 168, regs
    # the 8-wave instantiations keep two waves per SIMD
    assert all(n <= 256 for n in regs.values()), regs
    assert r.stderr.count("ScratchSize [bytes/lane]:") == r.stderr.count("ScratchSize [bytes/lane]: 0 ") > 0
