"""MI355X-native differentiable Gaussian-splatting rasterizer (LucidDreamer hot path)."""
__version__ = "0.1.0"


def install(*args, **kwargs):
    """Switch an unchanged LucidDreamer caller onto the fused pieces of this library in one call (luciddreamer_amd/dropin.py)."""
    from .dropin import install as _install
    return _install(*args, **kwargs)


def uninstall(handle):
    from .dropin import uninstall as _uninstall
    return _uninstall(handle)


def __getattr__(name):
    """`luciddreamer_amd.mcmc` (MCMCStrategy: relocation, capped growth, position noise), `luciddreamer_amd.filter3d` (the 3D
    smoothing filter of Mip-Splatting), `luciddreamer_amd.reproject` (point-cloud reprojection: warped frames and hole masks),
    `luciddreamer_amd.normals` (normals from depth and the normal losses), `luciddreamer_amd.smooth` (edge-aware smoothness of
    a rendered depth or normal map), `luciddreamer_amd.tsdf` (TSDF fusion of rendered
    depth and mesh extraction) and `luciddreamer_amd.mesh` (connected components, cluster filter and vertex normals of a mesh)
    without importing torch with the package."""
    if name in ("mcmc", "filter3d", "reproject", "normals", "smooth", "tsdf", "mesh"):
        import importlib
        return importlib.import_module("." + name, __name__)
    if name in ("fit_scale", "scatter_interpolate", "compensate", "dream_step"):     # dreaming on the device (reproject.py)
        import importlib
        return getattr(importlib.import_module(".reproject", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
