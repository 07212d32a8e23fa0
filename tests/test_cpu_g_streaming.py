"""No GPU: the host side of the runtime-size stream - the sizing and the refusals of nws_g_stream_step that are
decided before any device work (host arithmetic on the descriptor: no pointer is followed), the error a CPU-resident model gets,
and the stream class's public surface."""
import ctypes as C
import importlib
import inspect
import os
import re

import pytest

from g_stream_models import build

PKG = "neural-waveshaping-synthesis_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, BAD_ARG, WORKSPACE = -1, -2, -3     # include/nws_hip.h


def _lib():
    return importlib.import_module(PKG + "._lib")


def descriptor(**over):
    """a NwsGenericModel of the `bank` sizes whose pointers are a non-NULL dummy: enough for everything decided on the host"""
    lib = _lib()
    g = lib.NwsGenericModel()
    sizes = dict(control_size=2, gru_hidden=128, embedding=128, n_harmonics=40, n_shapers=12, hop=128, newt_mlp_depth=4, hgen_depth=4,
                 hgen_hidden=128, fir_len=256, out_channels=1, ir_len=31999, ln_eps=1e-5, leaky_slope=0.01)
    sizes.update(over)
    for k, v in sizes.items():
        setattr(g, k, v)
    p = 0x1000
    for name in ("gru_w_ih", "gru_w_hh", "gru_b_ih", "gru_b_hh", "proj_w", "proj_b", "mixer_w", "mixer_b", "newt_out_w", "newt_out_b",
                 "noise_window", "ir"):
        setattr(g, name, p)
    for name in ("newt_mlp_w", "newt_mlp_b", "newt_ln_g", "newt_ln_b", "hgen_w", "hgen_b", "hgen_ln_g", "hgen_ln_b"):
        for i in range(8):
            getattr(g, name)[i] = p
    g.shaper.n_shapers, g.shaper.width, g.shaper.depth, g.shaper.in_scale = sizes["n_shapers"], 16, 3, p
    for i in range(3):
        g.shaper.w[i] = g.shaper.b[i] = p
    return g


def test_state_bytes_grow_with_the_sizes_and_are_zero_when_refused():
    L = _lib().lib()
    g = descriptor()
    nb = lambda m, B, K, ir=None: L.nws_g_stream_state_bytes(C.byref(m), B, K, m.ir_len if ir is None else ir, None)
    base = nb(g, 1, 2)
    assert base > 4 * 65536                                    # at least the reverb-input ring of one row
    assert nb(g, 2, 2) > base and nb(g, 1, 4) > base and nb(g, 16, 16) > nb(g, 2, 16) > nb(g, 2, 4)
    assert nb(descriptor(out_channels=2), 1, 2) > base and nb(descriptor(gru_hidden=64), 1, 2) < base
    for bad in (dict(hop=64), dict(fir_len=128), dict(ir_len=32768), dict(ir_len=44099), dict(gru_hidden=0), dict(n_shapers=0),
                dict(embedding=700)):
        assert nb(descriptor(**bad), 1, 2) == 0, bad
    assert nb(g, 0, 2) == 0 and nb(g, 1, 0) == 0 and nb(g, 70000, 2) == 0 and nb(g, 1, 2, ir=1000) == 0
    assert L.nws_g_stream_state_bytes(None, 1, 2, 31999, None) == 0
    broken = descriptor()
    broken.mixer_w = None
    assert nb(broken, 1, 2) == 0


def test_argument_refusals_that_need_no_device():
    """every refusal is decided before the first launch, so these return without a device: dummy pointers are never followed"""
    L = _lib().lib()
    g = descriptor()
    B, maxf, K = 1, 4, 2
    nbytes = L.nws_g_stream_state_bytes(C.byref(g), B, maxf, g.ir_len, None)
    p = 0x1000

    def call(m=g, state=p, nb=nbytes, f0=p, control=p, Cn=2, k=K, first=1, seen=0, sr=16000.0, pu=p, rp=p, nz_new=None, nz_all=p, out=p,
             b=B):
        return L.nws_g_stream_step(C.byref(m) if m is not None else None, None, None, None, state, nb, b, maxf, f0, control, Cn, k, first,
                                   0, seen, 0, sr, pu, rp, nz_new, nz_all, 1024, out, None, None)

    assert call(m=None) == BAD_ARG
    for kw in (dict(state=None), dict(f0=None), dict(control=None), dict(pu=None), dict(rp=None), dict(out=None), dict(k=0), dict(k=maxf + 1),
               dict(b=0), dict(Cn=1), dict(first=1, seen=5), dict(first=0, seen=0), dict(nz_new=p), dict(nz_all=None), dict(sr=0.0)):
        assert call(**kw) == BAD_ARG, kw
    for bad in (dict(hop=64), dict(fir_len=128), dict(ir_len=40000)):
        assert call(m=descriptor(**bad)) == UNSUPPORTED, bad
    assert call(nb=nbytes - 4) == WORKSPACE
    # a chunk beyond 2048 samples needs the FFT reverb's plan
    big = L.nws_g_stream_state_bytes(C.byref(g), B, 32, g.ir_len, None)
    assert L.nws_g_stream_step(C.byref(g), None, None, None, p, big, B, 32, p, p, 2, 31, 1, 0, 0, 0, 16000.0, p, p, None, p, 1024, p, None,
                               None) == BAD_ARG
    assert L.nws_g_stream_reverb_tail(C.byref(g), None, p, p, p, nbytes, B, maxf, p, p, 1 << 20, None) == BAD_ARG


def test_entry_points_declared_and_bound():
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "nws_hip.h")).read()
    for name in ("nws_g_stream_state_bytes", "nws_g_stream_step", "nws_g_stream_reverb_tail"):
        assert re.search(rf"\b{name}\(", hdr) and name in lib.EXPORTED_SYMBOLS
    assert lib.ABI_VERSION == 6 and re.search(r"#define NWS_ABI_VERSION 6\b", hdr)


def test_cpu_resident_model_gets_the_no_cpu_fallback_error():
    model, _ = build("bank", False, device="cpu")
    assert not model._engine.specialised()
    with pytest.raises(RuntimeError, match="no CPU fallback") as e:
        model.stream(1)
    assert "fused kernels" not in str(e.value)
    with pytest.raises(RuntimeError, match="fused kernels"):
        model.stream(1, slots=True)                            # slot mode keeps today's text


def test_public_surface_equals_the_packaged_stream():
    st = importlib.import_module(PKG + ".streaming")
    assert issubclass(st.GenericNewtStream, st._StreamBase)
    for name in ("__init__", "push", "static_io", "hop", "refresh", "reverb_tail"):
        assert inspect.signature(getattr(st.GenericNewtStream, name)) == inspect.signature(getattr(st.NewtStream, name)), name
    # only what depends on the path is overridden: the path itself
    own = {k for k in vars(st.GenericNewtStream) if not k.startswith("__")}
    assert own == {"_PATH"} and st.GenericNewtStream._PATH is st._GenericPath and st.NewtStream._PATH is st._FusedPath


def test_the_two_paths_have_one_surface():
    st = importlib.import_module(PKG + ".streaming")
    public = lambda cls: {k: inspect.signature(v) for k, v in vars(cls).items() if not k.startswith("_") and callable(v)}
    fused, generic = public(st._FusedPath), public(st._GenericPath)
    assert fused == generic
    assert set(fused) == {"record", "rewalk", "settle", "reverb_aux", "state_bytes", "slot_state_bytes", "step", "step_slots",
                          "reverb_tail", "gave_up"}
    assert inspect.signature(st._FusedPath.__init__) == inspect.signature(st._GenericPath.__init__)


NO_CPU = ("{}gru.weight_ih_l0 lives on cpu: the NEWT forward path only runs as HIP kernels on an AMD GPU (move the model and inputs "
          "with .to('cuda')); there is no CPU fallback.")
FUSED_ONLY = "stateful streaming runs on the fused kernels: the model must have the architecture of gin/models/newt.gin"
SLOTS_HINT = " - model.voices(B) gives the slot stream of any architecture"


def test_each_stream_class_keeps_its_refusal_of_a_cpu_model():
    """The four constructors called directly on CPU-resident models: the path's construction-time refusal comes first, word for
    word (the fused path names the parameter as the packaged engine does, the runtime-size path as the descriptor does)."""
    nws = importlib.import_module(PKG)
    st = importlib.import_module(PKG + ".streaming")
    bank, _ = build("bank", False, device="cpu")
    nws.ensure_default_config()
    packaged = nws.NeuralWaveshaping().eval()
    assert packaged._engine.specialised() and not bank._engine.specialised()
    expected = {(st.NewtStream, packaged): NO_CPU.format("embedding."), (st.VoiceStream, packaged): NO_CPU.format("embedding."),
                (st.GenericNewtStream, packaged): NO_CPU.format(""), (st.GenericVoiceStream, packaged): NO_CPU.format(""),
                (st.NewtStream, bank): FUSED_ONLY, (st.VoiceStream, bank): FUSED_ONLY + SLOTS_HINT,
                (st.GenericNewtStream, bank): NO_CPU.format(""), (st.GenericVoiceStream, bank): NO_CPU.format("")}
    for (cls, model), text in expected.items():
        with pytest.raises(RuntimeError) as e:
            cls(model, 2)
        assert str(e.value) == text, cls.__name__
