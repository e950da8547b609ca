"""CPU: the opt-in antialiasing of the rasteriser (include/gpsgs.h GSR_FLAG_ANTIALIAS) -- the flag, the library's answer to
gsr_supported_flags(), the keyword on every entry point, the CPU-tensor refusal, and the fp64 statement of k the GPU tests use (tests/aa_ref.py)."""
import inspect
import re

import numpy as np
import pytest
import torch

from gps_gaussian_amd import _capi

from aa_ref import H_DIL, RHO_MIN, aa_k, aa_partials

import capi_run


def _flags():
    src = capi_run.header()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(GSR_FLAG_[A-Z_]+)\s+(\d+)u\b", src)}


def test_flag_value_mirror_and_no_overlap():
    flags = _flags()
    assert flags["GSR_FLAG_ANTIALIAS"] == 1024 == _capi.GSR_FLAG_ANTIALIAS
    others = [v for k, v in flags.items() if k != "GSR_FLAG_ANTIALIAS"]
    assert not any(v & 1024 for v in others)
    assert not 1024 & 0xF0  # the GSR_FLAG_TIMING_STAGE field


def test_library_lists_the_flag():
    lib = capi_run.lib()
    sup = lib.gsr_supported_flags()
    assert sup & _capi.GSR_FLAG_ANTIALIAS
    for name, v in _flags().items():  # every flag the header defines is one the library honours
        assert sup & v == v, name
    assert not sup & 0xF0
    assert lib.gpsgs_abi_version() == 4


def test_keyword_defaults_are_off():
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import render_api
    from gps_gaussian_amd.session import RasterSession
    for fn in (RZ.rasterize_gaussians, RZ.GaussianRasterizer.forward, render_api.render, render_api.render_ex, render_api.pts2render,
               RasterSession.__init__):
        p = inspect.signature(fn).parameters
        assert "antialiasing" in p and p["antialiasing"].default is False, fn.__qualname__
    assert "antialiasing" not in RZ.GaussianRasterizationSettings._fields and len(RZ.GaussianRasterizationSettings._fields) == 12


def _cpu_call(use_settings_attr):
    from gps_gaussian_amd import rasterizer as RZ
    rs, kw = capi_run.cpu_view()
    if use_settings_attr:
        from collections import namedtuple
        S = namedtuple("S", RZ.GaussianRasterizationSettings._fields + ("antialiasing",))
        rs = S(*rs, True)
    else:
        kw["antialiasing"] = True
    return RZ.GaussianRasterizer(rs)(**kw)


@pytest.mark.parametrize("how", ["keyword", "settings_attribute"])
def test_cpu_tensors_refused_like_any_call(how):
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        _cpu_call(how == "settings_attribute")


def test_cpu_tensors_refused_through_rasterize_gaussians():
    from gps_gaussian_amd import rasterizer as RZ
    rs, kw = capi_run.cpu_view()
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        RZ.rasterize_gaussians(kw["means3D"], kw["means2D"], None, kw["colors_precomp"], kw["opacities"], kw["scales"], kw["rotations"], None, rs,
                               antialiasing=True)


def test_k_partials_match_finite_differences_and_closed_form():
    rng = np.random.default_rng(3)
    n = 200
    a0 = torch.from_numpy(rng.uniform(0.05, 20.0, n))
    c0 = torch.from_numpy(rng.uniform(0.05, 20.0, n))
    b = torch.from_numpy(rng.uniform(-0.9, 0.9, n)) * torch.sqrt(a0 * c0)
    x = [t.clone().requires_grad_(True) for t in (a0, b, c0)]
    k, rho = aa_k(*x)
    assert (rho > RHO_MIN).all()
    g = torch.autograd.grad(k.sum(), x)
    closed = aa_partials(a0, b, c0)
    for j in range(3):
        want = closed[j] / (2.0 * k.detach())
        np.testing.assert_allclose(g[j].numpy(), want.numpy(), rtol=1e-12, atol=0)
        eps = 1e-6 * (1.0 + x[j].detach().abs())
        up = [t.detach().clone() for t in x]
        dn = [t.detach().clone() for t in x]
        up[j] += eps
        dn[j] -= eps
        fd = (aa_k(*up)[0] - aa_k(*dn)[0]) / (2 * eps)
        np.testing.assert_allclose(fd.numpy(), want.numpy(), rtol=1e-5, atol=1e-9)


def test_k_isotropic_closed_form_and_floor():
    s2 = torch.tensor([1e-4, 1e-3, 0.01, 0.1, 0.7, 1.0, 4.0, 100.0], dtype=torch.float64)
    k, rho = aa_k(s2, torch.zeros_like(s2), s2)
    want = s2 / (s2 + H_DIL)  # det ratio (s2 / (s2 + h))^2, square root
    live = want ** 2 > RHO_MIN
    np.testing.assert_allclose(k[live].numpy(), want[live].numpy(), rtol=1e-14)
    np.testing.assert_allclose(k[~live].numpy(), 0.005, rtol=1e-14)
    assert (~live).sum() >= 2 and 0.005 > 1.0 / 255.0
    # below the floor -- a slightly negative a0 c0 - b^2 from rounding included -- k is the constant 0.005 and has no gradient
    x = [torch.tensor([1.0], dtype=torch.float64, requires_grad=True), torch.tensor([1.0 + 1e-12], dtype=torch.float64, requires_grad=True),
         torch.tensor([1.0], dtype=torch.float64, requires_grad=True)]
    kk, r = aa_k(*x)
    assert float(r) < 0 and float(kk) == pytest.approx(0.005, rel=1e-14)
    assert all(float(t) == 0.0 for t in torch.autograd.grad(kk.sum(), x))
