"""CPU: GPSGS_ACCELERATE=splat serves this package's stand-in for the reference's lib/TaichiRender.py (which imports taichi and cannot load on
this card), so the reference's UNMODIFIED train_stage1.py imports; "all" keeps meaning the five fused features; the splat refuses CPU tensors.

Each hook case runs in a fresh interpreter with the integration path, the harness of hook_run.py; those skip where there is no
reference checkout."""
import pytest
import torch

import hook_run as H


@H.needs_ref
def test_train_stage1_imports_with_the_splat_substitute(tmp_path):
    out = H.run("""
        import train_stage1 as T                           # the reference's script, unmodified, imported (not run)
        import gps_gaussian_amd.splat as SP, gps_gaussian_amd.accelerate as A
        import lib.TaichiRender
        assert T.TaichiRenderBatch is SP.TaichiRenderBatch, T.TaichiRenderBatch
        assert lib.TaichiRender.TaichiRenderBatch is SP.TaichiRenderBatch
        assert "taichi" not in sys.modules
        assert A.installed() == {"lib.TaichiRender.TaichiRenderBatch": "splat"}, A.installed()
        print("SERVED")
    """, "splat", tmp_path)
    assert "SERVED" in out


@H.needs_ref
def test_all_plus_splat_binds_both(tmp_path):
    out = H.run("""
        import train_stage1 as T
        import gps_gaussian_amd.splat as SP, gps_gaussian_amd.accelerate as A
        import core.corr, gps_gaussian_amd.corr as MC
        assert T.TaichiRenderBatch is SP.TaichiRenderBatch
        assert issubclass(core.corr.CorrBlockFast1D, MC.CorrBlockFast1D)
        feats = set(A.installed().values())
        assert "splat" in feats and {"corr", "upsample", "unproject"} <= feats, feats   # train_stage1 never imports lib.GaussianRender (pack)
        print("BOTH")
    """, "all,splat", tmp_path)
    assert "BOTH" in out


@H.needs_ref
def test_without_the_variable_the_reference_module_is_not_served(tmp_path):
    out = H.run("""
        import importlib.util
        import gps_gaussian_amd.accelerate as A
        import lib.network  # noqa: F401  (imports corr_sampler: the drop-in, where the hook would install itself)
        assert not [f for f in sys.meta_path if type(f).__module__ == A.__name__]
        spec = importlib.util.find_spec("lib.TaichiRender")
        assert spec is not None and spec.origin.endswith(os.path.join("lib", "TaichiRender.py")), spec
        try:
            import lib.TaichiRender  # noqa: F401
        except ImportError as e:   # the reference's own file: taichi is not installed here
            print("REFERENCE", type(e).__name__)
        else:
            print("REFERENCE loaded")
    """, None, tmp_path)
    assert "REFERENCE" in out


@H.needs_ref
def test_all_alone_does_not_serve_the_substitute(tmp_path):
    out = H.run("""
        import lib.network  # noqa: F401
        import importlib.util
        spec = importlib.util.find_spec("lib.TaichiRender")
        assert spec.origin.endswith(os.path.join("lib", "TaichiRender.py")), spec
        print("NOT SERVED")
    """, "all", tmp_path)
    assert "NOT SERVED" in out


def test_all_means_the_five_features_and_splat_is_opt_in():
    import gps_gaussian_amd  # noqa: F401
    from gps_gaussian_amd import accelerate as A
    assert A.requested("all") == A.FEATURES and "splat" not in A.FEATURES
    assert A.requested("all,splat") == A.FEATURES + ("splat",)
    assert A.requested("splat") == ("splat",) and A.requested("splat,loss") == ("loss", "splat")
    assert A.requested("") == () and "splat" in A.calls
    with pytest.raises(ValueError):
        A.requested("all,splta")


def test_cpu_tensors_raise_the_gpu_error():
    import gps_gaussian_amd  # noqa: F401
    from gps_gaussian_amd import splat
    pts = torch.zeros(1, 1, 4, 6)
    mask = torch.ones(1, 1, 4)
    depth = torch.zeros(1, 8, 8)
    color = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        splat.zsplat(pts, mask, depth, color)
    view = {"flow_pred": torch.zeros(1, 1, 8, 8), "mask": torch.ones(1, 1, 8, 8), "img": torch.zeros(1, 3, 8, 8)}
    data = {"lmain": view, "rmain": dict(view), "novel_view": {"intr": torch.eye(3)[None], "extr": torch.zeros(1, 3, 4)}}
    with pytest.raises(RuntimeError, match="GPU"):
        splat.TaichiRenderBatch(bs=1, res=8).flow2render(data)
