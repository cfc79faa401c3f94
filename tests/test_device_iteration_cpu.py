"""CPU-side checks of the counted training step (ngm_render_*_counted): the three symbols are declared, exported and
listed, and the two checks that are specific to them -- a NULL count, a configuration outside the counted step -- answer
before anything else is looked at, so they can be reached without a GPU (the structs handed in are ctypes mirrors whose
pointers the host never dereferences)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngm_hip.h")
COUNTED = ("ngm_render_fwd_counted", "ngm_render_bwd_counted", "ngm_render_bwd_adam_counted")


@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build(verbose=False)
    return _capi


def test_counted_symbols_declared_exported_listed(capi):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = capi.lib()
    for n in COUNTED:
        plain = n[:-len("_counted")]
        m = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{n} is not declared in include/ngm_hip.h"
        mp = re.search(r"\bint\s+" + plain + r"\s*\(([^;]*)\)\s*;", src)
        args, pargs = [a.strip() for a in m.group(1).split(",")], [a.strip() for a in mp.group(1).split(",")]
        # <arguments of the plain call>, const int32_t* num_active
        assert len(args) == len(pargs) + 1 and re.sub(r"\s+", " ", args[-1]) == "const int32_t* num_active"
        assert [re.sub(r"\s+", " ", a).rsplit(" ", 1)[0] for a in args[:-1]] == \
               [re.sub(r"\s+", " ", a).rsplit(" ", 1)[0] for a in pargs]
        assert hasattr(L, n), f"{n} is not exported by the library"
        assert n in capi.EXPORTED
        assert len(getattr(L, n).argtypes) == len(getattr(L, plain).argtypes) + 1
    # an addition: the ABI number and the comment that explains it
    head = open(HEADER).read()
    assert int(re.search(r"#define\s+NGM_ABI_VERSION\s+(\d+)", head).group(1)) == 11 == L.ngm_abi_version()
    assert "ngm_render_fwd_counted" in re.search(r"#define\s+NGM_ABI_VERSION[^\n]*", head).group(0)


def _call(capi, name, fc, rc, count):
    """the counted call `name` with dummy structs / pointers and `count` as num_active"""
    L = capi.lib()
    ps, rays, tg, pred, gr = capi.Params(), capi.Rays(), capi.Targets(), capi.Prediction(), capi.Grads()
    b = C.byref
    if name == "ngm_render_fwd_counted":
        return L.ngm_render_fwd_counted(b(fc), b(rc), b(ps), b(rays), b(tg), b(pred), None, None, 0, None, count)
    if name == "ngm_render_bwd_counted":
        return L.ngm_render_bwd_counted(b(fc), b(rc), b(ps), b(rays), b(tg), b(pred), None, b(gr), None, None, 0, None, count)
    one = (capi.AdamTensor * 1)()
    return L.ngm_render_bwd_adam_counted(b(fc), b(rc), b(ps), b(rays), b(tg), b(pred), None, b(gr), one, 1, None, None, 1, None,
                                         1e-3, 0.9, 0.999, 1e-15, 0.0, None, None, 0, None, count)


@pytest.mark.parametrize("name", COUNTED)
def test_counted_specific_validation_without_gpu(capi, name):
    L = capi.lib()
    fc = capi.field_cfg(encoding="fourier", dim_enc=64, num_layers=2)
    rc = capi.render_cfg()
    dummy = 0x1000                      # a "device pointer" the host must not dereference
    # NULL count
    assert _call(capi, name, fc, rc, None) == capi.NGM_E_INVALID
    err = L.ngm_last_error()
    assert name.encode() in err and b"num_active is NULL" in err
    # configurations outside the counted step: UNSUPPORTED, each with its reason
    outside = [(fc, capi.render_cfg(geometry_mode="neus"), b"neus"),
               (capi.field_cfg(encoding="triplane", num_components=16, resolution=8), rc, b"triplane"),
               (fc, capi.render_cfg(photometric_loss="gaussian_nll"), b"_nll"),
               (fc, capi.render_cfg(depth_loss="gaussian_nll"), b"_nll"),
               (fc, capi.render_cfg(depth_loss="laplacian_nll"), b"_nll")]
    for f, r, word in outside:
        assert _call(capi, name, f, r, dummy) == capi.NGM_E_UNSUPPORTED
        err = L.ngm_last_error()
        assert name.encode() in err and word in err and b"counted step" in err
        # the NULL count is reported first
        assert _call(capi, name, f, r, None) == capi.NGM_E_INVALID
    # a configuration inside the counted step gets past both checks: the ordinary validation of the plain call answers
    # (empty ngm_params: NGM_E_INVALID with its own message), still without a launch
    assert _call(capi, name, fc, rc, dummy) == capi.NGM_E_INVALID
    assert b"num_active" not in L.ngm_last_error() and b"counted step" not in L.ngm_last_error()


def test_renderer_draws_the_same_line_as_the_library(capi):
    """NeuralGraphRenderer.counted_step_unsupported (host side: it decides about the warned fallback) and the library's
    check (NGM_E_UNSUPPORTED of ngm_render_fwd_counted) agree on every configuration, inside and outside the counted step"""
    from types import SimpleNamespace
    from neural_graph_mapping_amd import renderer as R
    assert hasattr(R.NeuralGraphRenderer, "capture_training")
    assert "count" in R.DeviceTarget._fields and issubclass(R.DeviceTarget, R.Target.__bases__[0])
    fourier = capi.field_cfg(encoding="fourier", dim_enc=64, num_layers=2)
    cases = [(fourier, capi.render_cfg()), (capi.field_cfg(encoding="permuto", num_layers=1), capi.render_cfg()),
             (capi.field_cfg(encoding="nerf", num_octaves=8, num_layers=1, skip_mode="concat"), capi.render_cfg(geometry_mode="density")),
             (fourier, capi.render_cfg(photometric_loss="l2")),
             (fourier, capi.render_cfg(geometry_mode="neus")),
             (capi.field_cfg(encoding="triplane", num_components=16, resolution=8), capi.render_cfg()),
             (fourier, capi.render_cfg(photometric_loss="gaussian_nll")), (fourier, capi.render_cfg(depth_loss="gaussian_nll")),
             (fourier, capi.render_cfg(depth_loss="laplacian_nll"))]
    refused = 0
    for fc, rc in cases:
        host = R.NeuralGraphRenderer.counted_step_unsupported(SimpleNamespace(_fc=fc, _rc_train=rc))
        code = _call(capi, "ngm_render_fwd_counted", fc, rc, 0x1000)
        assert (host is not None) == (code == capi.NGM_E_UNSUPPORTED), (host, code, capi.lib().ngm_last_error())
        refused += host is not None
    assert refused == 5
