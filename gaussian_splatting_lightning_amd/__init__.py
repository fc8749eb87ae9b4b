"""MI355X-native differentiable Gaussian rasterizer (drop-in for `diff_gaussian_rasterization`).

The hot path of pomelyu/gaussian_splatting_lightning -- preprocess, binning, compositing and their
backward -- runs in hand-written HIP kernels for gfx950 (csrc/), exposed through the C ABI in
include/gsrast.h and bound here with ctypes.  See DESIGN.md.
"""
from .rasterizer import (GaussianRasterizationSettings, GaussianRasterizer, mark_visible,  # noqa: F401
                         rasterize_contributions, rasterize_gaussians)
from .bilagrid import BilateralGrid, slice_image, total_variation_loss  # noqa: F401
from .normals import (depth_to_normal, geometry_features, normal_consistency,  # noqa: F401
                      render_normal_consistency)

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "rasterize_contributions",
           "mark_visible", "BilateralGrid", "slice_image", "total_variation_loss", "geometry_features",
           "normal_consistency", "depth_to_normal", "render_normal_consistency"]
