"""CPU: the host side of the diffusion trunk's fp16 mode (option "trunk_fp16" = the reference's DiffusionTts.enable_fp16 / config
use_fp16, vqvae/diff_model.py:143-157, 299-309) - argument checks that must fire before any device work, the config key reaching the
option, the C ABI, and the reference fixture's own figures (trunk_fp16.npz, make_golden_fp16.py)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoDevice:
    """a model whose runtime must never be touched"""
    @property
    def rt(self):
        raise AssertionError("device work before the arguments were checked")


class _OptionsOnly:
    """a runtime that answers option queries and fails on anything that would launch"""

    def __init__(self, **opts):
        self.opts = {"conv_x3": 1, "trunk_fp16": 0, **opts}
        self.calls = []

    def get_option(self, key):
        return self.opts[key]

    def set_option(self, key, value):
        self.calls.append((key, int(value)))
        self.opts[key] = int(value)

    def __getattr__(self, name):
        raise AssertionError(f"device work ({name}) before the arguments were checked")


def _entry_points():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return (SynthesizerTrn.infer, lambda self, *a, **k: next(SynthesizerTrn.infer_stream(self, [{}], **k)))


def test_trunk_precision_arg():
    from detail_tts_amd.vqvae.model_24k import trunk_precision_arg
    assert trunk_precision_arg(None) is None and trunk_precision_arg("fp32") == 0 and trunk_precision_arg("fp16") == 1
    for bad in ("bf16", "FP16", 16, True, ""):
        with pytest.raises(ValueError, match="trunk_precision"):
            trunk_precision_arg(bad)


@pytest.mark.parametrize("bad", ["bf16", "half", 1])
def test_unknown_trunk_precision_rejected_before_any_launch(bad):
    for fn in _entry_points():
        with pytest.raises(ValueError, match="trunk_precision"):
            fn(_NoDevice(), None, None, None, None, trunk_precision=bad)


def test_fp16_with_exact_fp32_kernels_rejected_before_any_launch():
    """trunk_precision='fp16' has no meaning with conv_x3 = 0: refused after reading the option back, before anything else"""
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn

    class M:
        rt = _OptionsOnly(conv_x3=0)

    for fn in _entry_points():
        with pytest.raises(ValueError, match="conv_x3"):
            fn(M(), None, None, None, None, trunk_precision="fp16")
    assert M.rt.calls == []


def test_per_call_precision_is_restored_even_when_the_diffusion_fails():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn

    class M:
        _trunk_precision = SynthesizerTrn._trunk_precision
        rt = _OptionsOnly()

    m = M()
    with pytest.raises(RuntimeError):
        with m._trunk_precision(1):
            assert m.rt.opts["trunk_fp16"] == 1
            raise RuntimeError("diffusion failed")
    assert m.rt.opts["trunk_fp16"] == 0 and m.rt.calls == [("trunk_fp16", 1), ("trunk_fp16", 0)]
    m.rt.calls.clear()
    with m._trunk_precision(None):               # no per-call value: the option is not touched
        pass
    assert m.rt.calls == []
    m.rt.opts["trunk_fp16"] = 1                  # a model whose config says use_fp16: a per-call "fp32" gives it back afterwards
    with m._trunk_precision(0):
        assert m.rt.opts["trunk_fp16"] == 0
    assert m.rt.opts["trunk_fp16"] == 1


def test_config_use_fp16_reaches_the_option():
    """diffusion.use_fp16 of a config in the reference's format -> DiffusionTts.enable_fp16 -> option trunk_fp16; default: untouched"""
    from detail_tts_amd.config import load_config
    from detail_tts_amd.vqvae.diff_model import DiffusionTts
    assert load_config()["diffusion"]["use_fp16"] is False
    rt = _OptionsOnly()
    d = DiffusionTts(rt, load_config()["diffusion"])
    assert rt.calls == [] and d.enable_fp16 is False
    cfg = load_config({"diffusion": {"use_fp16": True}})
    assert cfg["diffusion"]["use_fp16"] is True and cfg["diffusion"]["model_channels"] == 768
    rt = _OptionsOnly()
    d = DiffusionTts(rt, cfg["diffusion"])
    assert rt.calls == [("trunk_fp16", 1)] and d.enable_fp16 is True
    d.enable_fp16 = False                        # settable as on the reference's module
    assert rt.calls[-1] == ("trunk_fp16", 0) and d.enable_fp16 is False


def test_c_abi_declares_and_exports_the_option_entry():
    from detail_tts_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "detail_hip.h")).read()
    assert re.search(r"int\s+dtts_get_option\s*\(\s*dtts_handle\s*\*\s*h\s*,\s*const\s+char\s*\*\s*key\s*,\s*int\s*\*\s*value\s*\)", hdr)
    assert '"trunk_fp16"' in hdr and "vqvae/diff_model.py:143-157, 299-309" in hdr
    assert "dtts_get_option" in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdetail_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert hasattr(lib, "dtts_get_option") and hasattr(lib, "dtts_set_option")


def test_reference_fixture_has_nonzero_errors(golden):
    """E_ref = |reference enable_fp16 run - reference fp32 run| of every case is there and non-zero (autocast engaged), and of the
    size bf16 gives (1e-3 .. 5e-2 on outputs of magnitude ~1)"""
    g = golden("trunk_fp16")
    keys = [k for k in g if k.endswith("_emax")]
    fwd = [k for k in keys if k.startswith("fwd")]
    assert len(fwd) == 8 and {"e2e_mel_emax", "e2e_wav_emax"} <= set(keys)
    for k in keys:
        assert float(g[k]) > 0 and float(g[k[:-5] + "_erel"]) > 0, k
    for k in fwd:
        assert 1e-3 < float(g[k]) < 5e-2 and 1e-3 < float(g[k[:-5] + "_erel"]) < 5e-2, (k, float(g[k]))
    for t in g["fwd48_timesteps"]:
        for nm in ("cond", "uncond"):
            y32, y16 = g[f"fwd48_t{int(t)}_{nm}_y32"], g[f"fwd48_t{int(t)}_{nm}_y16"]
            assert np.isclose(float(np.max(np.abs(y16.astype(np.float64) - y32))), float(g[f"fwd48_t{int(t)}_{nm}_emax"]), rtol=1e-6)
    f = golden("diff_forward")                   # the fixture's fp32 run IS the existing fp32 fixture
    t0 = int(f["ts"][0])
    assert np.array_equal(g[f"fwd48_t{t0}_cond_y32"], f["out_cond"]) and np.array_equal(g[f"fwd48_t{t0}_uncond_y32"], f["out_uncond"])
