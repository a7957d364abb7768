"""langsplat_amd -- MI355X-native differentiable Gaussian rasterizer for LangSplat.

The hot path (forward + backward of RasterizeGaussians, BASELINE.json north_star) is
implemented as HIP kernels for gfx950 in csrc/, exposed through the C ABI of include/lsr.h
(liblsr.so) and wrapped here with the reference's Python API.
"""
from .lerf_eval import activate_stream, evaluate_frame, lerf_localization, smooth_relevancy  # noqa: F401
from .loss import rgb_loss, ssim  # noqa: F401
from .levels import LevelsStep, render_levels, render_levels_train, split_levels, stack_levels  # noqa: F401
from .levels_graph import GraphedLevelsStep, LevelsViewSlot  # noqa: F401
from .query import Decoder, decode, relevancy_map, render_levels_relevancy, render_relevancy  # noqa: F401
from .query import label_stats, render_levels_semantic, render_semantic, semantic_map  # noqa: F401
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians  # noqa: F401

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians",
           "Decoder", "decode", "relevancy_map", "render_relevancy",
           "stack_levels", "split_levels", "render_levels", "render_levels_train", "LevelsStep",
           "GraphedLevelsStep", "LevelsViewSlot",
           "render_levels_relevancy",
           "smooth_relevancy", "activate_stream", "lerf_localization", "evaluate_frame",
           "rgb_loss", "ssim"]
