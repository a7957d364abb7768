"""ctypes binding of liblsr.so (the C ABI in include/lsr.h).

This is the reference-side binding a maintainer would add in place of the CUDA extension's
pybind module `diff_gaussian_rasterization._C`.  Tensors are passed as raw
device pointers; scratch buffers are torch uint8 tensors handed out through the allocator
callback (so the caching allocator owns them and autograd keeps them alive for backward).

There is no CPU fallback: if liblsr.so cannot be loaded the import of this module fails.
"""
from __future__ import annotations

import ctypes
import math
import os
import threading
from typing import Dict, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# LSR_LIB: a measurement variant built by tools/build_variant.py (same-box A/B); default the product
LIB_PATH = os.environ.get("LSR_LIB") or os.path.join(_HERE, "liblsr.so")

LSR_BUF_GEOM, LSR_BUF_BINNING, LSR_BUF_IMAGE, LSR_BUF_BACKWARD, LSR_BUF_LEVELS = 0, 1, 2, 3, 4
MAX_LEVELS = 4  # include/lsr.h LSR_MAX_LEVELS
ABI_VERSION = 18
ADAM_STEP_WORDS = 66  # include/lsr.h LSR_ADAM_STEP_WORDS
ADAM_WORD_SKIPPED, ADAM_WORD_LR = 49, 50  # LSR_ADAM_WORD_SKIPPED / LSR_ADAM_WORD_LR
# lsr_raw_flags (include/lsr.h): inputs are GaussianModel's raw parameters
RAW_OPACITY, RAW_SCALES, RAW_ROTATIONS, RAW_LANGUAGE = 1, 2, 4, 8
FWD_ZERO_GRAD_RECORDS, FWD_NO_COLOR_GRAD, FWD_NO_BACKWARD = 1, 2, 4  # lsr_forward_flags
BWD_RECORDS_ZEROED, BWD_SHARED_CU, BWD_DEFER_TAIL = 1, 2, 4  # lsr_backward_flags
_vp = ctypes.c_void_p


class LsrSettings(ctypes.Structure):
    _fields_ = [
        ("image_height", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("tanfovx", ctypes.c_float),
        ("tanfovy", ctypes.c_float),
        ("scale_modifier", ctypes.c_float),
        ("sh_degree", ctypes.c_int32),
        ("prefiltered", ctypes.c_int32),
        ("debug", ctypes.c_int32),
        ("include_feature", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("bg", _vp),
        ("viewmatrix", _vp),
        ("projmatrix", _vp),
        ("campos", _vp),
    ]


class LsrForwardArgs(ctypes.Structure):
    _fields_ = [("P", ctypes.c_int32), ("M", ctypes.c_int32)] + [
        (n, _vp) for n in ("means3D", "shs", "colors_precomp", "language_feature", "opacities", "scales",
                           "rotations", "cov3D_precomp", "out_color", "out_language_feature", "radii")
    ] + [("raw", ctypes.c_int32), ("flags", ctypes.c_int32), ("shs_rest", _vp), ("visible", _vp),
         ("loss_target", _vp), ("loss_mask", _vp), ("out_loss", _vp), ("capacity_rendered", ctypes.c_int64),
         ("capacity_entries", ctypes.c_int64), ("overflow", _vp), ("out_num_entries", ctypes.POINTER(ctypes.c_int64)),
         ("language_ready", _vp), ("phase", ctypes.c_int32)]


class LsrForwardLevelsArgs(ctypes.Structure):
    _fields_ = [("fwd", LsrForwardArgs), ("levels", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("more_language_feature", _vp), ("more_out_language_feature", _vp)]


class LsrBackwardLevelsArgs(ctypes.Structure):
    _fields_ = [("P", ctypes.c_int32), ("levels", ctypes.c_int32), ("raw", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("num_rendered", ctypes.c_int64)] + [
        (n, _vp) for n in ("geom_buffer", "binning_buffer", "image_buffer", "radii", "language_feature",
                           "dL_dout_language_feature", "out_language_feature", "loss_target", "loss_mask",
                           "dL_dloss", "scratch", "dL_dlanguage_feature")]


class LsrAdamTensor(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp),
                ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("step", ctypes.c_int64)]


class LsrLevelsStepForwardArgs(ctypes.Structure):
    _fields_ = [("levels", LsrForwardLevelsArgs), ("reserved", ctypes.c_int32)]


class LsrLevelsStepBackwardArgs(ctypes.Structure):
    _fields_ = LsrBackwardLevelsArgs._fields_ + [
        ("update", ctypes.POINTER(LsrAdamTensor)), ("update_step_dev", _vp), ("update_skip", _vp),
        ("fill_record", _vp), ("fill_levels", _vp), ("reserved2", ctypes.c_int64)]


class LsrBackwardArgs(ctypes.Structure):
    _fields_ = [("P", ctypes.c_int32), ("M", ctypes.c_int32), ("num_rendered", ctypes.c_int64)] + [
        (n, _vp) for n in ("means3D", "shs", "colors_precomp", "language_feature", "opacities", "scales",
                           "rotations", "cov3D_precomp", "radii", "dL_dout_color", "dL_dout_language_feature",
                           "geom_buffer", "binning_buffer", "image_buffer", "dL_dmeans2D", "dL_dcolors",
                           "dL_dlanguage_feature", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
                           "dL_dscales", "dL_drotations")
    ] + [("raw", ctypes.c_int32), ("flags", ctypes.c_int32), ("shs_rest", _vp), ("dL_dsh_rest", _vp),
         ("dL_dloss", _vp), ("update", ctypes.POINTER(LsrAdamTensor)), ("update_step_dev", _vp),
         ("update_skip", _vp), ("fill_record", _vp)]


class LsrStateLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in (
        "depth_key", "tiles_touched", "rect", "record", "clamped", "sorted_ids", "super_offset",
        "counters", "ranges", "final_T", "n_contrib", "point_list", "grad_records")]


class LsrViewPlanOffsets(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in (
        "pack_counters", "pack_cover", "pack_bytes",
        "set_counters", "set_cover", "set_final_T", "set_n_contrib", "set_split_desc", "set_bwd_lists",
        "set_loss_code",
        "tiles", "classes", "split_items", "word_plan_ready", "word_bwd_class")]


class LsrKernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("launches", ctypes.c_int64), ("total_ms", ctypes.c_double)]


class LsrQueryArgs(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int64), ("feature", _vp), ("channel_stride", ctypes.c_int64),
                ("pixel_stride", ctypes.c_int64), ("n_layers", ctypes.c_int32),
                ("widths", ctypes.POINTER(ctypes.c_int32)), ("weights", _vp), ("n_pos", ctypes.c_int32),
                ("n_neg", ctypes.c_int32), ("phrases", _vp), ("out_relevancy", _vp), ("out_decoded", _vp)]


class LsrQuerySemanticArgs(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int64), ("feature", _vp), ("channel_stride", ctypes.c_int64),
                ("pixel_stride", ctypes.c_int64), ("n_layers", ctypes.c_int32),
                ("widths", ctypes.POINTER(ctypes.c_int32)), ("weights", _vp), ("n_labels", ctypes.c_int32),
                ("n_neg", ctypes.c_int32), ("phrases", _vp), ("out_label", _vp), ("out_score", _vp)]


class LsrLabelStatsArgs(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int64), ("n_maps", ctypes.c_int32), ("gt_maps", ctypes.c_int32),
                ("n_classes", ctypes.c_int32), ("pred", _vp), ("gt", _vp), ("out_counts", _vp), ("out_totals", _vp)]


class LsrEvalStats(ctypes.Structure):
    _fields_ = [("blend_min", ctypes.c_float), ("blend_max", ctypes.c_float), ("avg_max", ctypes.c_float),
                ("avg_argmax", ctypes.c_int32)]


class LsrEvalFilterArgs(ctypes.Structure):
    _fields_ = [("n_maps", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("maps", _vp),
                ("out_avg", _vp), ("out_blend", _vp), ("out_stats", _vp)]


class LsrEvalMaskArgs(ctypes.Structure):
    _fields_ = [("n_maps", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("blend", _vp),
                ("stats", _vp), ("thresh", ctypes.c_float), ("n_prompts", ctypes.c_int32), ("gt_mask", _vp),
                ("out_mask", _vp), ("out_mask_raw", _vp), ("out_counts", _vp)]


RGB_LOSS_TILE = (32, 32)  # include/lsr.h LSR_RGB_LOSS_TILE_H, LSR_RGB_LOSS_TILE_W


class LsrRgbLossArgs(ctypes.Structure):
    _fields_ = [("planes", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("lambda_dssim", ctypes.c_float), ("image", _vp), ("target", _vp), ("out_terms", _vp),
                ("out_maps", _vp), ("out_ssim_map", _vp), ("scratch", _vp)]


class LsrRgbLossBwdArgs(ctypes.Structure):
    _fields_ = [("planes", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("lambda_dssim", ctypes.c_float), ("image", _vp), ("target", _vp), ("maps", _vp),
                ("dL_dloss", _vp), ("out_dL_dimage", _vp)]


class LsrViewArgs(ctypes.Structure):
    _fields_ = [("P", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("fused_loss", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("capacity_rendered", ctypes.c_int64), ("capacity_entries", ctypes.c_int64),
                ("num_rendered", ctypes.c_int64), ("geom", _vp), ("image", _vp), ("binning", _vp), ("radii", _vp),
                ("pack", _vp), ("pack_bytes", ctypes.c_size_t), ("overflow", _vp)]


ALLOC_FN = ctypes.CFUNCTYPE(_vp, _vp, ctypes.c_int32, ctypes.c_size_t)

# symbol -> (restype, argtypes); must cover every function declared in include/lsr.h
SIGNATURES = {
    "lsr_abi_version": (ctypes.c_int32, []),
    "lsr_last_error": (ctypes.c_char_p, []),
    "lsr_geom_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "lsr_image_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "lsr_binning_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]),
    "lsr_backward_bytes": (ctypes.c_size_t, [ctypes.c_int32]),
    "lsr_state_layout_of": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                             ctypes.POINTER(LsrStateLayout)]),
    "lsr_forward": (ctypes.c_int32, [ctypes.POINTER(LsrSettings), ctypes.POINTER(LsrForwardArgs), ALLOC_FN, _vp,
                                     _vp, ctypes.POINTER(ctypes.c_int64)]),
    "lsr_backward": (ctypes.c_int32, [ctypes.POINTER(LsrSettings), ctypes.POINTER(LsrBackwardArgs), ALLOC_FN, _vp,
                                      _vp]),
    "lsr_levels_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "lsr_debug_levels_occupancy": (ctypes.c_int32, [ctypes.c_int32]),
    "lsr_forward_levels": (ctypes.c_int32, [ctypes.POINTER(LsrSettings), ctypes.POINTER(LsrForwardLevelsArgs),
                                            ALLOC_FN, _vp, _vp, ctypes.POINTER(ctypes.c_int64)]),
    "lsr_backward_levels_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "lsr_backward_levels": (ctypes.c_int32, [ctypes.POINTER(LsrSettings), ctypes.POINTER(LsrBackwardLevelsArgs), _vp]),
    "lsr_levels_step_forward": (ctypes.c_int32, [ctypes.POINTER(LsrSettings), ctypes.POINTER(LsrLevelsStepForwardArgs),
                                                 ALLOC_FN, _vp, _vp, ctypes.POINTER(ctypes.c_int64)]),
    "lsr_levels_step_backward": (ctypes.c_int32, [ctypes.POINTER(LsrSettings),
                                                  ctypes.POINTER(LsrLevelsStepBackwardArgs), _vp]),
    "lsr_mark_visible": (ctypes.c_int32, [ctypes.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "lsr_query_relevancy": (ctypes.c_int32, [ctypes.POINTER(LsrQueryArgs), _vp]),
    "lsr_query_semantic": (ctypes.c_int32, [ctypes.POINTER(LsrQuerySemanticArgs), _vp]),
    "lsr_label_stats": (ctypes.c_int32, [ctypes.POINTER(LsrLabelStatsArgs), _vp]),
    "lsr_eval_filter": (ctypes.c_int32, [ctypes.POINTER(LsrEvalFilterArgs), _vp]),
    "lsr_eval_masks": (ctypes.c_int32, [ctypes.POINTER(LsrEvalMaskArgs), _vp]),
    "lsr_rgb_loss_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "lsr_rgb_loss_forward": (ctypes.c_int32, [ctypes.POINTER(LsrRgbLossArgs), _vp]),
    "lsr_rgb_loss_backward": (ctypes.c_int32, [ctypes.POINTER(LsrRgbLossBwdArgs), _vp]),
    "lsr_view_pack_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]),
    "lsr_view_plan_pack_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]),
    "lsr_view_plan_layout": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.POINTER(LsrViewPlanOffsets)]),
    "lsr_view_counts": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp]),
    "lsr_view_save": (ctypes.c_int32, [ctypes.POINTER(LsrViewArgs), _vp]),
    "lsr_view_restore": (ctypes.c_int32, [ctypes.POINTER(LsrViewArgs), _vp]),
    "lsr_view_bind_layout": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
    "lsr_view_bind": (ctypes.c_int32, [ctypes.POINTER(LsrViewArgs), ctypes.c_int32, _vp]),
    "lsr_fill_language_plane": (ctypes.c_int32, [ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp, _vp]),
    "lsr_adam_fill_language_plane": (ctypes.c_int32, [ctypes.POINTER(LsrAdamTensor), ctypes.c_float, _vp, _vp, _vp,
                                                      ctypes.c_int32, _vp]),
    "lsr_fill_language": (ctypes.c_int32, [ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp, _vp]),
    "lsr_adam_step": (ctypes.c_int32, [ctypes.c_int64, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_double, ctypes.c_int64, _vp]),
    "lsr_adam_multi": (ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(LsrAdamTensor), ctypes.c_float, _vp, _vp,
                                        _vp]),
    "lsr_adam_fill_language": (ctypes.c_int32, [ctypes.POINTER(LsrAdamTensor), ctypes.c_float, _vp, _vp, _vp,
                                                ctypes.c_int32, _vp]),
    "lsr_language_tail": (ctypes.c_int32, [ctypes.POINTER(LsrSettings), ctypes.POINTER(LsrBackwardArgs), _vp]),
    "lsr_densification_stats": (ctypes.c_int32, [ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsr_dist_cuda2": (ctypes.c_int32, [ctypes.c_int64, _vp, _vp, ALLOC_FN, _vp, _vp]),
    "lsr_debug_knn_grid": (ctypes.c_int32, [ctypes.POINTER(ctypes.c_float), ctypes.c_int64,
                                            ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)]),
    "lsr_masked_l1_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int64]),
    "lsr_masked_l1_forward": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp,
                                               _vp]),
    "lsr_masked_l1_backward": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int32, _vp,
                                                _vp, _vp]),
    "lsr_decode_language_feature": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp,
                                                     ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp,
                                                     _vp]),
    "lsr_debug_scan_stalls": (ctypes.c_int32, []),
    "lsr_debug_set_spin_limit": (ctypes.c_uint32, [ctypes.c_uint32]),
    "lsr_debug_bucket_timeline": (ctypes.c_int32, [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int32]),
    "lsr_debug_clock_probe": (ctypes.c_int32, [_vp, _vp]),
    "lsr_graph_launch": (ctypes.c_int32, [_vp, _vp, ctypes.POINTER(_vp), ctypes.c_int32, _vp]),
    "lsr_debug_render_stats": (ctypes.c_int32, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32]),
    "lsr_debug_render_timeline": (ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int32]),
    "lsr_profile_enable": (ctypes.c_int32, [ctypes.c_int32]),
    "lsr_profile_report": (ctypes.c_int32, [ctypes.POINTER(LsrKernelStat), ctypes.c_int32]),
    "lsr_profile_select": (ctypes.c_int32, [ctypes.c_char_p]),
    "lsr_profile_sample": (ctypes.c_int32, [ctypes.c_int32]),
}

# the bound form of the view cache (include/lsr.h lsr_view_bind): added without an ABI bump, so a
# library of the same ABI may lack them; has_view_bind() says whether they are there
OPTIONAL = ("lsr_view_bind_layout", "lsr_view_bind", "lsr_fill_language_plane", "lsr_adam_fill_language_plane")
# the walk plan (include/lsr.h lsr_view_plan_pack_bytes), additive in the same way: has_view_plan()
OPTIONAL_PLAN = ("lsr_view_plan_pack_bytes", "lsr_view_plan_layout")
# test hooks added the same way (include/lsr.h lsr_debug_knn_grid)
OPTIONAL_DEBUG = ("lsr_debug_knn_grid",)
BIND_FORWARD, BIND_BACKWARD, BIND_FILL_PLANE, BIND_CLAMPED = 16, 16, 32, 1

_lib: Optional[ctypes.CDLL] = None


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load liblsr.so (building it first if it is absent and hipcc is available)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        from . import build as _build  # compiles the HIP sources; not a fallback path
        _build.build()
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if name in OPTIONAL + OPTIONAL_PLAN + OPTIONAL_DEBUG and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.lsr_abi_version() != ABI_VERSION:
        raise RuntimeError("liblsr.so ABI version mismatch")
    _lib = lib
    return lib


_autograd = None


def autograd_helper():
    """The _lsr_autograd extension (csrc/lsr_autograd.cpp: a leaf tensor's cached AccumulateGrad node,
    read and released; host code), built in-tree first if it is absent."""
    global _autograd
    if _autograd is None:
        if not os.path.exists(os.path.join(_HERE, "_lsr_autograd.so")):
            from . import build as _build
            _build.build_autograd_helper()
        from . import _lsr_autograd
        _autograd = _lsr_autograd
    return _autograd


def last_error() -> str:
    return load().lsr_last_error().decode(errors="replace")


def _check(status: int, what: str):
    if status != 0:
        raise RuntimeError(f"{what} failed (status {status}): {last_error()}")


class GraphLauncher:
    """One captured graph's launch on one stream after given events, with an event recorded after it
    (lsr_graph_launch): the raw handles are read once, so a call costs one ctypes round trip instead
    of torch's stream context, event waits and CUDAGraph.replay() (pipeline.py's synced replays)."""

    def __init__(self, graph: "torch.cuda.CUDAGraph", stream: "torch.cuda.Stream", waits, record):
        self._lib = load()
        self._exec = _vp(graph.raw_cuda_graph_exec())
        if not self._exec.value:
            raise RuntimeError("GraphLauncher: the graph has no instantiated executable")
        self._stream = _vp(stream.cuda_stream)
        self._events = list(waits) + [record]  # kept alive with their handles
        self._waits = (_vp * max(1, len(waits)))(*[e.cuda_event for e in waits])
        self._n = len(waits)
        self._record = _vp(record.cuda_event) if record is not None else None

    def __call__(self):
        _check(self._lib.lsr_graph_launch(self._exec, self._stream, self._waits, self._n, self._record),
               "lsr_graph_launch")


def _ptr(t: Optional[torch.Tensor]):
    if t is None or t.numel() == 0:
        return None
    return ctypes.c_void_p(t.data_ptr())


def _stream(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _Allocator:
    """Hands out torch uint8 device tensors for the ABI's scratch requests.

    One process-wide ctypes callback (creating a CFUNCTYPE per call costs more than the whole
    binding); the allocator active on this thread is published through a thread-local.
    """

    _tls = threading.local()

    def __init__(self, device: torch.device):
        self.device = device
        self.buffers: Dict[int, torch.Tensor] = {}

    def __enter__(self):
        self._prev = getattr(_Allocator._tls, "active", None)
        _Allocator._tls.active = self
        return self

    def __exit__(self, *exc):
        _Allocator._tls.active = self._prev

    def get(self, which: int) -> torch.Tensor:
        t = self.buffers.get(which)
        return t if t is not None else torch.empty((0,), dtype=torch.uint8, device=self.device)


def _alloc_cb(user, which, nbytes):
    a = getattr(_Allocator._tls, "active", None)
    if a is None:
        return None
    try:
        n = max(int(nbytes), 1)
        st = static_buffers.active()
        t = st.tensor(("scratch", int(which)), (n,), torch.uint8, a.device, at_least=True) if st is not None \
            else torch.empty((n,), dtype=torch.uint8, device=a.device)
    except Exception:  # noqa: BLE001 -- reported to C as NULL -> LSR_ERR_ALLOC
        return None
    a.buffers[int(which)] = t
    return t.data_ptr()


_ALLOC_CB = ALLOC_FN(_alloc_cb)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t if t.is_contiguous() else t.contiguous()


class _on_device:
    """torch.cuda.device(...) only when it is not already the current device."""

    def __init__(self, device: torch.device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self.ctx = None if idx == torch.cuda.current_device() else torch.cuda.device(idx)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


class capacity:
    """Within the block, the rasterizer forwards of this thread run in capacity mode (include/lsr.h
    lsr_forward_args.capacity_*): buffers and launch grids sized from `rendered` tile instances and
    `entries` super-tile entries, no wait for the device -- what a HIP graph capture of the step needs
    (langsplat_amd.graph).  `overflow`: a () int32 device tensor each forward sets to 0, or when its
    view exceeds a capacity (it is then not rasterized) to the bits of 1.0f (non-zero as an int; 1.0
    through overflow.view(torch.float32), which GradBucket.all_reduce(flag=) reduces over ranks)."""

    _tls = threading.local()

    def __init__(self, rendered: int, entries: int, overflow: torch.Tensor):
        if rendered <= 0 or entries <= 0:
            raise ValueError("capacity: both capacities must be positive")
        if overflow.dtype != torch.int32 or overflow.numel() != 1:
            raise ValueError("capacity: overflow must be a one-element int32 tensor")
        self.rendered, self.entries, self.overflow = int(rendered), int(entries), overflow

    @staticmethod
    def active():
        return getattr(capacity._tls, "cur", None)

    def __enter__(self):
        self._prev = capacity.active()
        capacity._tls.cur = self
        return self

    def __exit__(self, *exc):
        capacity._tls.cur = self._prev


class language_ready:
    """Within the block, the rasterizer forwards of this thread defer the language feature
    (include/lsr.h lsr_forward_args.language_ready): preprocess, depth order and binning run at
    once, and the stream waits for `event` (a torch.cuda.Event recorded after the language feature's
    last update, on any stream) only before the feature enters the records and the compositing
    starts.  event None: off (the block is a no-op)."""

    _tls = threading.local()

    def __init__(self, event):
        self.event = event

    @staticmethod
    def active():
        return getattr(language_ready._tls, "cur", None)

    def __enter__(self):
        self._prev = language_ready.active()
        language_ready._tls.cur = self.event
        return self

    def __exit__(self, *exc):
        language_ready._tls.cur = self._prev


class forward_phase:
    """Within the block, the rasterizer forwards of this thread enqueue one half of the forward
    (include/lsr.h lsr_forward_args.phase; capacity mode only): GEOMETRY = preprocess, depth order
    and binning; COMPOSITE = the language feature into the records, the compositing and the fused
    loss, into the buffers the geometry call of the same static_buffers set wrote; COMPOSITE_FILLED =
    the same without the feature fill (a fused update wrote the records' language slots: fused_update
    with fill)."""

    GEOMETRY, COMPOSITE, COMPOSITE_FILLED = 1, 2, 3
    _tls = threading.local()

    def __init__(self, phase: int):
        if phase not in (0, 1, 2, 3):
            raise ValueError("forward_phase: 0 (all), 1 (geometry), 2 (composite) or 3 (composite, feature "
                             "already in the records)")
        self.phase = int(phase)

    @staticmethod
    def active() -> int:
        return getattr(forward_phase._tls, "cur", 0)

    def __enter__(self):
        self._prev = forward_phase.active()
        forward_phase._tls.cur = self.phase
        return self

    def __exit__(self, *exc):
        forward_phase._tls.cur = self._prev


class static_buffers:
    """Within the block, the rasterizer forwards of this thread put their scratch buffers and output
    tensors into this object's persistent tensors instead of fresh allocations: the same addresses at
    every forward.  A pipelined graph step (langsplat_amd.pipeline.PipelinedGraphStep) captures a
    backward that reads what a forward captured in ANOTHER graph writes, so both must name the same
    memory.  Tensors are (re)allocated only when a request does not fit (never during a capture)."""

    _tls = threading.local()

    def __init__(self):
        self.tensors: Dict[tuple, torch.Tensor] = {}
        # the bound form (include/lsr.h lsr_view_bind): this set's split-phase forwards and their
        # backwards read the records and the point list through the set's table
        self.view_bind = False

    @staticmethod
    def active():
        return getattr(static_buffers._tls, "cur", None)

    def tensor(self, key, shape, dtype, device, at_least=False):
        """The persistent tensor `key` of `shape` (at_least: a 1-D tensor of at least shape[0] elements,
        a view of its first shape[0])."""
        t = self.tensors.get(key)
        fits = t is not None and t.dtype == dtype and t.device == torch.device(device) and (
            t.numel() >= shape[0] if at_least else tuple(t.shape) == tuple(shape))
        if not fits:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"static_buffers: {key} {tuple(shape)} does not fit during a capture")
            t = torch.empty(shape, dtype=dtype, device=device)
            self.tensors[key] = t
        return t[:shape[0]] if at_least else t

    def __enter__(self):
        self._prev = static_buffers.active()
        static_buffers._tls.cur = self
        return self

    def __exit__(self, *exc):
        static_buffers._tls.cur = self._prev


class fused_update:
    """Within the block, a language-only rasterizer backward of `param` (the raw _language_feature,
    the fused-activation path) also applies `optimizer`'s Adam step to it in the same pass
    (include/lsr.h lsr_backward_args.update; train.py:104 + 134-137 at N = 1), and optimizer.step()
    then leaves it alone.  The optimizer must be a langsplat_amd.optim.Adam prepared for a capture
    (its device step block; only inside a graph capture) with `param` its one parameter.  skip: its
    skip flag (the overflow flag); fill: a device pointer to another forward's record array whose
    language slots receive the updated activated feature (langsplat_amd.pipeline), or None.

    defer=True (N > 1, include/lsr.h LSR_BWD_DEFER_TAIL): the backward runs the render backward only
    and leaves the per-Gaussian language partials in its geometry buffer; partials() is that (P, 3)
    tensor, which the caller all-reduces (AVG over the ranks), then run_tail() launches the rest in
    one pass -- the gradient outputs, the Adam step and the fill (lsr_language_tail).  The backward's
    returned gradients hold their values only after run_tail()."""

    # process-wide, not thread-local: autograd runs a CUDA node's backward on its device thread, not
    # on the thread that called loss.backward()
    _cur = None

    def __init__(self, optimizer, param: torch.Tensor, skip: Optional[torch.Tensor] = None, fill: Optional[int] = None,
                 defer: bool = False, fill_plane: bool = False):
        self.optimizer, self.param, self.skip, self.fill = optimizer, param, skip, fill
        self.fill_plane = bool(fill_plane)  # fill is a set's plane (LSR_BIND_FILL_PLANE), not its records
        self.defer = bool(defer)
        self.used = False
        self.pending = None  # defer: the deferred tail's arguments (and every tensor they point into)

    def partials(self) -> torch.Tensor:
        """defer: what the caller all-reduces -- the deferred backward's 3 P language partials and the
        step's skip word after them, (3 P + 1,) fp32, a view of its buffer (include/lsr.h)."""
        if self.pending is None:
            raise RuntimeError("fused_update.partials: no deferred backward ran in this block")
        return self.pending[3]

    def run_tail(self):
        """defer: lsr_language_tail on the current stream, after the caller reduced partials()."""
        if self.pending is None:
            raise RuntimeError("fused_update.run_tail: no deferred backward ran in this block")
        s, a, _keep, part, device = self.pending
        if part.numel() == 0:
            return
        with _on_device(device):
            _check(load().lsr_language_tail(ctypes.byref(s), ctypes.byref(a), _stream(device)), "lsr_language_tail")

    @staticmethod
    def active():
        return fused_update._cur

    def __enter__(self):
        self._prev = fused_update._cur
        fused_update._cur = self
        return self

    def __exit__(self, *exc):
        fused_update._cur = self._prev

    def table(self):
        """The lsr_adam_tensor of the update (the optimizer's state and group hyper-parameters)."""
        opt, p = self.optimizer, self.param
        gi = next(i for i, g in enumerate(opt.param_groups) if any(q is p for q in g["params"]))
        g = opt.param_groups[gi]
        st = opt.state[p]
        beta1, beta2 = g["betas"]
        opt._register_fused(gi)
        return LsrAdamTensor(p.numel(), p.data_ptr(), None, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             float(g["lr"]), float(beta1), float(beta2), float(g["eps"]), opt.step_offset(p))


def output_tensor(key, shape, dtype, device) -> torch.Tensor:
    """An output tensor of the rasterizer forward: the active static_buffers' persistent one, else new."""
    st = static_buffers.active()
    if st is None:
        return torch.empty(shape, dtype=dtype, device=device)
    # a fresh alias of the persistent tensor: the autograd Function that returns it sets ITS grad_fn,
    # so the persistent tensor never keeps an autograd graph (and the parameters' AccumulateGrad
    # nodes, bound to the capture stream) alive past the step that produced it
    return st.tensor(("out", key), shape, dtype, device).detach()


# (P, W, H) -> (tile instances, super-tile entries) of this thread's last forward outside capacity mode
# (the capacities a later capture needs)
LAST_COUNTS: Dict[tuple, tuple] = {}


_SETTINGS_CACHE: Dict[int, tuple] = {}


def make_settings(rs, keep: list) -> LsrSettings:
    """lsr_settings from a GaussianRasterizationSettings (gaussian_renderer/__init__.py:37-51).

    Cached per settings object (a NamedTuple, so immutable): render() builds one per view and the
    forward and backward both convert it.  The cache holds the object, so its id stays unique."""
    hit = _SETTINGS_CACHE.get(id(rs))
    if hit is not None and hit[0] is rs:
        keep.append(hit[2])
        return hit[1]
    mine: list = []
    s = _build_settings(rs, mine)
    if len(_SETTINGS_CACHE) >= 16:
        _SETTINGS_CACHE.clear()
    _SETTINGS_CACHE[id(rs)] = (rs, s, mine)
    keep.append(mine)
    return s


def _build_settings(rs, keep: list) -> LsrSettings:
    s = LsrSettings()
    s.image_height = int(rs.image_height)
    s.image_width = int(rs.image_width)
    s.tanfovx = float(rs.tanfovx)
    s.tanfovy = float(rs.tanfovy)
    s.scale_modifier = float(rs.scale_modifier)
    s.sh_degree = int(rs.sh_degree)
    s.prefiltered = int(bool(rs.prefiltered))
    s.debug = int(bool(rs.debug))
    s.include_feature = int(bool(getattr(rs, "include_feature", False)))
    for name in ("bg", "viewmatrix", "projmatrix", "campos"):
        t = _f32c_cached(getattr(rs, name))
        keep.append(t)
        setattr(s, name, t.data_ptr())
    return s


_CONTIG_CACHE: Dict[int, tuple] = {}


def _f32c_cached(src: torch.Tensor) -> torch.Tensor:
    """_f32c of a camera tensor, reused while the source object and its version are unchanged.

    render() builds new settings every step from the same camera tensors, and the reference's
    world_view_transform is a transposed view (scene/cameras.py:47): without the cache every step
    pays a small copy kernel for it."""
    t = src.detach()
    if t.dtype == torch.float32 and t.is_contiguous():
        return t
    hit = _CONTIG_CACHE.get(id(src))
    if hit is not None and hit[0] is src and hit[1] == src._version:
        return hit[2]
    c = _f32c(t)
    if len(_CONTIG_CACHE) >= 64:
        _CONTIG_CACHE.clear()
    _CONTIG_CACHE[id(src)] = (src, src._version, c)
    return c


def _fill_forward_args(a: LsrForwardArgs, means3D, shs, colors_precomp, language_feature, opacities, scales,
                       rotations, cov3D_precomp, raw, flags, shs_rest, out_color, out_language, radii, visible):
    """The fields of lsr_forward_args every forward sets: the counts P and M (shs_rest included), the
    raw and forward flags, the inputs, the outputs and the optional visibility output."""
    a.P = int(means3D.shape[0])
    a.M = int(shs.shape[1]) if shs is not None and shs.numel() > 0 else 0
    if shs_rest is not None and shs_rest.numel() > 0:
        a.M += int(shs_rest.shape[1])
        a.shs_rest = _ptr(shs_rest)
    a.raw = int(raw)
    a.flags = int(flags)
    a.means3D = _ptr(means3D)
    a.shs = _ptr(shs)
    a.colors_precomp = _ptr(colors_precomp)
    a.language_feature = _ptr(language_feature)
    a.opacities = _ptr(opacities)
    a.scales = _ptr(scales)
    a.rotations = _ptr(rotations)
    a.cov3D_precomp = _ptr(cov3D_precomp)
    a.out_color = _ptr(out_color)
    a.out_language_feature = _ptr(out_language)
    a.radii = _ptr(radii)
    a.visible = _ptr(visible)


def forward_bound() -> bool:
    """As this thread's contexts stand, a rasterizer forward is made in the bound form (include/lsr.h
    LSR_BIND_FORWARD): a split phase in capacity mode into a static_buffers set with view_bind.  The
    caller of that forward keeps the answer with its backward's state and passes BIND_BACKWARD in the
    backward's flags (langsplat_amd.rasterizer does, in the autograd context)."""
    st = static_buffers.active()
    return st is not None and st.view_bind and forward_phase.active() != 0 and capacity.active() is not None


def rasterize_gaussians(rs, means3D, shs, colors_precomp, language_feature, opacities, scales, rotations,
                        cov3D_precomp, raw=0, shs_rest=None, visible=None, loss_target=None, loss_mask=None,
                        out_loss=None, flags=0):
    """Native forward: returns (num_rendered, color, language_feature_image, radii, geom, binning, image).

    raw / shs_rest: the fused-activation form (include/lsr.h lsr_raw_flags); shs is then
    features_dc (P,1,3) and shs_rest features_rest (P,M-1,3).  visible: optional (P,) bool tensor
    that receives radii > 0.  out_loss: optional () fp32 tensor that receives the fused
    l1_loss(lang * mask, loss_target * mask) (loss_target (3,H,W) fp32, loss_mask H*W bool)."""
    lib = load()
    device = means3D.device
    P = int(means3D.shape[0])
    H, W = int(rs.image_height), int(rs.image_width)
    keep: list = []
    s = make_settings(rs, keep)
    color = output_tensor("color", (3, H, W), torch.float32, device)
    lang = output_tensor("language", (3, H, W), torch.float32, device)
    radii = output_tensor("radii", (P,), torch.int32, device)  # preprocess writes every entry
    if visible is not None and (visible.dtype != torch.bool or visible.numel() != P or not visible.is_contiguous()):
        raise ValueError("visible must be a contiguous (P,) bool tensor")
    a = LsrForwardArgs()
    _fill_forward_args(a, means3D, shs, colors_precomp, language_feature, opacities, scales, rotations,
                       cov3D_precomp, raw, flags, shs_rest, color, lang, radii, visible)
    if out_loss is not None:
        if loss_target is None or tuple(loss_target.shape) != (3, H, W) or loss_target.dtype != torch.float32 \
                or not loss_target.is_contiguous():
            raise ValueError("loss_target must be a contiguous (3,H,W) fp32 tensor")
        if loss_mask is None or loss_mask.dtype != torch.bool or loss_mask.numel() != H * W \
                or not loss_mask.is_contiguous():
            raise ValueError("loss_mask must be a contiguous bool tensor of H*W elements")
        a.loss_target = _ptr(loss_target)
        a.loss_mask = _ptr(loss_mask)
        a.out_loss = _ptr(out_loss)
    cap = capacity.active()
    entries = ctypes.c_int64(0)
    ready = language_ready.active()
    if ready is not None and language_feature is not None:
        a.language_ready = ready.cuda_event
        keep.append(ready)
    a.phase = forward_phase.active()
    if forward_bound():
        a.flags |= BIND_FORWARD
    if cap is not None:
        a.capacity_rendered = cap.rendered
        a.capacity_entries = cap.entries
        a.overflow = _ptr(cap.overflow)
    else:
        a.out_num_entries = ctypes.pointer(entries)
    alloc = _Allocator(device)
    nr = ctypes.c_int64(0)
    with _on_device(device), alloc:
        _check(lib.lsr_forward(ctypes.byref(s), ctypes.byref(a), _ALLOC_CB, None, _stream(device), ctypes.byref(nr)),
               "lsr_forward")
    if cap is None:
        LAST_COUNTS[(P, W, H)] = (int(nr.value), int(entries.value))
    elif a.phase == forward_phase.GEOMETRY and static_buffers.active() is not None:
        # what a lsr_view_restore into this set needs to stand in for this call (view_restore_args)
        static_buffers.active().geometry_call = dict(
            P=P, W=W, H=H, flags=int(flags), rendered=cap.rendered, entries=cap.entries, overflow=cap.overflow,
            fused_loss=int(out_loss is not None and bool(s.include_feature) and language_feature is not None))
    return (int(nr.value), color, lang, radii, alloc.get(LSR_BUF_GEOM), alloc.get(LSR_BUF_BINNING),
            alloc.get(LSR_BUF_IMAGE))


def check_level_features(language_features, P: int) -> int:
    """L of an (L, P, 3) stack of level features, 1 <= L <= MAX_LEVELS; anything else: ValueError."""
    if not isinstance(language_features, torch.Tensor) or language_features.dim() != 3 \
            or tuple(language_features.shape[1:]) != (P, 3) \
            or not 1 <= int(language_features.shape[0]) <= MAX_LEVELS:
        got = tuple(language_features.shape) if isinstance(language_features, torch.Tensor) else type(language_features)
        raise ValueError(f"language_features must have shape (L, P, 3) with 1 <= L <= {MAX_LEVELS} and P = {P}, "
                         f"got {got}")
    return int(language_features.shape[0])


def _fill_levels_forward_args(la: LsrForwardLevelsArgs, means3D, shs, colors_precomp, lf, opacities, scales, rotations,
                              cov3D_precomp, raw, shs_rest, color, langs, radii, visible):
    """lsr_forward_levels_args of either levels forward: the inference forward of level 0 (lf[0] into
    langs[0]) and, with more than one level, the rest of the contiguous (L, P, 3) stack lf and of langs."""
    _fill_forward_args(la.fwd, means3D, shs, colors_precomp, lf, opacities, scales, rotations, cov3D_precomp, raw,
                       FWD_NO_BACKWARD, shs_rest, color, langs, radii, visible)
    la.levels = int(lf.shape[0])
    if la.levels > 1:
        la.more_language_feature = _ptr(lf[1:])
        la.more_out_language_feature = _ptr(langs[1:])


def _fill_levels_backward_args(who: str, a, keep: list, L, H, W, radii, geom, binning, image, grad_images, images,
                               targets, masks, grad_losses):
    """The seeds (validated; ValueError in who's name), the forward's state buffers and radii of either
    levels backward's args struct; the tensors the call reads are appended to keep."""
    fused = [images, targets, masks, grad_losses]
    if any(x is not None for x in fused) and any(x is None for x in fused):
        raise ValueError(f"{who}: images, targets, masks and grad_losses go together")
    if grad_images is None and images is None:
        raise ValueError(f"{who}: no seed (grad_images or the fused seed)")
    for name, t in (("grad_images", grad_images), ("images", images), ("targets", targets)):
        if t is not None and tuple(t.shape) != (L, 3, H, W):
            raise ValueError(f"{who}: {name} must be ({L}, 3, {H}, {W}), got {tuple(t.shape)}")
    if grad_images is not None:
        keep.append(_f32c(grad_images.detach()))
        a.dL_dout_language_feature = keep[-1].data_ptr()
    if images is not None:
        if masks.dtype != torch.bool or tuple(masks.shape) != (L, H, W) or tuple(grad_losses.shape) != (L,):
            raise ValueError(f"{who}: masks must be ({L}, {H}, {W}) bool and grad_losses ({L},)")
        keep += [_f32c(images.detach()), _f32c(targets.detach()), masks.contiguous(), _f32c(grad_losses.detach())]
        a.out_language_feature, a.loss_target, a.loss_mask, a.dL_dloss = (t.data_ptr() for t in keep[-4:])
    a.geom_buffer, a.binning_buffer, a.image_buffer = _ptr(geom), _ptr(binning), _ptr(image)
    a.radii = _ptr(radii)


def rasterize_gaussians_levels(rs, means3D, shs, colors_precomp, language_features, opacities, scales, rotations,
                               cov3D_precomp, raw=0, shs_rest=None, with_visibility=False, keep_state=False):
    """All language levels of a scene in one inference forward (include/lsr.h lsr_forward_levels):
    language_features is (L, P, 3), 1 <= L <= MAX_LEVELS, raw iff raw has RAW_LANGUAGE; the other
    arguments are rasterize_gaussians'.  Returns (num_rendered, color (3, H, W), language_images
    (L, 3, H, W), radii), and with_visibility the (P,) bool radii > 0 after them.  Level l's image is
    bit-identical to rasterize_gaussians' for language_features[l].  keep_state: the forward's geometry,
    binning and image buffers after everything else, for rasterize_gaussians_levels_backward (the only
    backward of this forward); otherwise nothing is kept."""
    lib = load()
    device = means3D.device
    P = int(means3D.shape[0])
    L = check_level_features(language_features, P)
    H, W = int(rs.image_height), int(rs.image_width)
    keep: list = []
    s = make_settings(rs, keep)
    lf = _f32c(language_features.detach())
    color = torch.empty((3, H, W), dtype=torch.float32, device=device)
    langs = torch.empty((L, 3, H, W), dtype=torch.float32, device=device)
    radii = torch.empty((P,), dtype=torch.int32, device=device)  # preprocess writes every entry
    visible = torch.empty((P,), dtype=torch.bool, device=device) if with_visibility else None
    la = LsrForwardLevelsArgs()
    _fill_levels_forward_args(la, means3D, shs, colors_precomp, lf, opacities, scales, rotations, cov3D_precomp, raw,
                              shs_rest, color, langs, radii, visible)
    entries = ctypes.c_int64(0)
    la.fwd.out_num_entries = ctypes.pointer(entries)
    alloc = _Allocator(device)
    nr = ctypes.c_int64(0)
    with _on_device(device), alloc:
        _check(lib.lsr_forward_levels(ctypes.byref(s), ctypes.byref(la), _ALLOC_CB, None, _stream(device),
                                      ctypes.byref(nr)), "lsr_forward_levels")
    LAST_COUNTS[(P, W, H)] = (int(nr.value), int(entries.value))  # the capacities a later capture needs
    out = (int(nr.value), color, langs, radii)
    if with_visibility:
        out += (visible,)
    if keep_state:
        out += (alloc.get(LSR_BUF_GEOM), alloc.get(LSR_BUF_BINNING), alloc.get(LSR_BUF_IMAGE))
    return out


def rasterize_gaussians_levels_backward(rs, language_features, radii, num_rendered, geom, binning, image, raw=0,
                                        grad_images=None, images=None, targets=None, masks=None, grad_losses=None):
    """The language gradient of every level of a rasterize_gaussians_levels(..., keep_state=True) forward
    (include/lsr.h lsr_backward_levels): (L, P, 3), w.r.t. language_features (raw iff raw has
    RAW_LANGUAGE), zeros for culled Gaussians.  Seeds: grad_images (L, 3, H, W) = dL/d(the maps), and /
    or the fused masked-L1 seed of sum_l grad_losses[l] * l1_loss(images[l] * masks[l], targets[l] *
    masks[l]): images (the forward's maps) and targets (L, 3, H, W), masks (L, H, W) bool, grad_losses
    (L,), all four or none.  Both given: their sum."""
    lib = load()
    device = radii.device
    P = int(radii.shape[0])
    L = check_level_features(language_features, P)
    H, W = int(rs.image_height), int(rs.image_width)
    keep: list = []
    s = make_settings(rs, keep)
    a = LsrBackwardLevelsArgs()
    _fill_levels_backward_args("rasterize_gaussians_levels_backward", a, keep, L, H, W, radii, geom, binning, image,
                               grad_images, images, targets, masks, grad_losses)
    a.P, a.levels, a.raw, a.num_rendered = P, L, int(raw) & RAW_LANGUAGE, int(num_rendered)
    lf = _f32c(language_features.detach())
    a.language_feature = _ptr(lf)
    out = torch.empty((L, P, 3), dtype=torch.float32, device=device)
    scratch = torch.empty((int(lib.lsr_backward_levels_bytes(P, L)),), dtype=torch.uint8, device=device)
    a.scratch = _ptr(scratch)
    a.dL_dlanguage_feature = _ptr(out)
    with _on_device(device):
        _check(lib.lsr_backward_levels(ctypes.byref(s), ctypes.byref(a), _stream(device)), "lsr_backward_levels")
    return out


def levels_step_forward(rs, means3D, shs, colors_precomp, language_features, opacities, scales, rotations,
                        cov3D_precomp, raw=0, shs_rest=None):
    """rasterize_gaussians_levels without a host wait (include/lsr.h lsr_levels_step_forward): needs an
    active `capacity`, honours forward_phase (all, COMPOSITE, COMPOSITE_FILLED) and puts outputs and
    scratch into the active static_buffers, as rasterize_gaussians does -- so a rasterize_gaussians
    call in forward_phase.GEOMETRY (flags=FWD_NO_BACKWARD, language_features[0] as its feature) over the
    same static_buffers supplies a composite phase's geometry (radii and `visible` are written by the
    phase that runs the preprocess: give that call visible=output_tensor("visible", (P,), torch.bool,
    device), the tensor returned here).  Returns (capacity, color (3, H, W),
    language_images (L, 3, H, W), radii, visible (P,) bool, geom, binning, image, levels): the three
    state buffers and the LSR_BUF_LEVELS array (empty for L == 1), for levels_step_backward."""
    lib = load()
    device = means3D.device
    P = int(means3D.shape[0])
    L = check_level_features(language_features, P)
    cap = capacity.active()
    if cap is None:
        raise RuntimeError("levels_step_forward: capacity mode only (inside a _native.capacity block)")
    H, W = int(rs.image_height), int(rs.image_width)
    keep: list = []
    s = make_settings(rs, keep)
    lf = _f32c(language_features.detach())
    color = output_tensor("color", (3, H, W), torch.float32, device)
    langs = output_tensor("levels_language", (L, 3, H, W), torch.float32, device)
    radii = output_tensor("radii", (P,), torch.int32, device)
    visible = output_tensor("visible", (P,), torch.bool, device)
    sa = LsrLevelsStepForwardArgs()
    la = sa.levels
    _fill_levels_forward_args(la, means3D, shs, colors_precomp, lf, opacities, scales, rotations, cov3D_precomp, raw,
                              shs_rest, color, langs, radii, visible)
    la.fwd.phase = forward_phase.active()
    la.fwd.capacity_rendered = cap.rendered
    la.fwd.capacity_entries = cap.entries
    la.fwd.overflow = _ptr(cap.overflow)
    alloc = _Allocator(device)
    nr = ctypes.c_int64(0)
    with _on_device(device), alloc:
        _check(lib.lsr_levels_step_forward(ctypes.byref(s), ctypes.byref(sa), _ALLOC_CB, None, _stream(device),
                                           ctypes.byref(nr)), "lsr_levels_step_forward")
    return (int(nr.value), color, langs, radii, visible, alloc.get(LSR_BUF_GEOM), alloc.get(LSR_BUF_BINNING),
            alloc.get(LSR_BUF_IMAGE), alloc.get(LSR_BUF_LEVELS))


class LevelsUpdate:
    """levels_step_backward's fused Adam step (include/lsr.h lsr_levels_step_backward_args.update): the
    raw (L, P, 3) features `param` with their moments, the hyper-parameters, the device step block
    (int64[ADAM_STEP_WORDS]: the count, and at ADAM_WORD_LR the learning rate's bits) and this tensor's
    offset from its count, the optional skip flag (device int32) and the optional fill targets: a
    device address of render records (state_layout's "record" in a geometry buffer) and the
    LSR_BUF_LEVELS array of that forward (a uint8 tensor; needed with L > 1)."""

    def __init__(self, param, exp_avg, exp_avg_sq, betas, eps, step_dev, step_offset=0, skip=None, fill_record=None,
                 fill_levels=None):
        for t in (param, exp_avg, exp_avg_sq):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != param.shape or t.device != param.device:
                raise ValueError("LevelsUpdate: param, exp_avg and exp_avg_sq must be contiguous fp32 tensors of one "
                                 "shape on one device")
        if step_dev.dtype != torch.int64 or step_dev.numel() < ADAM_STEP_WORDS or step_dev.device != param.device:
            raise ValueError(f"LevelsUpdate: step_dev must be int64[{ADAM_STEP_WORDS}] on the features' device")
        if skip is not None and (skip.dtype != torch.int32 or skip.numel() != 1 or skip.device != param.device):
            raise ValueError("LevelsUpdate: skip must be a one-element int32 tensor on the features' device")
        self.param, self.exp_avg, self.exp_avg_sq = param, exp_avg, exp_avg_sq
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.step_dev, self.step_offset, self.skip = step_dev, int(step_offset), skip
        self.fill_record, self.fill_levels = fill_record, fill_levels

    def table(self) -> LsrAdamTensor:
        return LsrAdamTensor(self.param.numel(), self.param.data_ptr(), None, self.exp_avg.data_ptr(),
                             self.exp_avg_sq.data_ptr(), 0.0, self.betas[0], self.betas[1], self.eps, self.step_offset)


def levels_step_backward(rs, language_features, radii, num_rendered, geom, binning, image, raw=0, grad_images=None,
                         images=None, targets=None, masks=None, grad_losses=None, update: Optional[LevelsUpdate] = None,
                         out=None, scratch=None, want_grad=True):
    """rasterize_gaussians_levels_backward on a levels_step_forward's buffers, without a host wait
    (include/lsr.h lsr_levels_step_backward); num_rendered is what that forward returned (its capacity).
    update: the Adam step of language_features (and the next forward's feature fills) in the tail;
    language_features must then be update.param itself.  out / scratch: persistent tensors for the
    (L, P, 3) gradient and the accumulator (a captured step), else fresh ones; want_grad=False with
    update writes no gradient tensor (returns None)."""
    lib = load()
    device = radii.device
    P = int(radii.shape[0])
    L = check_level_features(language_features, P)
    H, W = int(rs.image_height), int(rs.image_width)
    keep: list = []
    s = make_settings(rs, keep)
    a = LsrLevelsStepBackwardArgs()
    _fill_levels_backward_args("levels_step_backward", a, keep, L, H, W, radii, geom, binning, image, grad_images,
                               images, targets, masks, grad_losses)
    a.P, a.levels, a.raw, a.num_rendered = P, L, int(raw) & RAW_LANGUAGE, int(num_rendered)
    if update is not None:
        if language_features is not update.param and language_features.data_ptr() != update.param.data_ptr():
            raise ValueError("levels_step_backward: with update, language_features is update.param")
        lf = update.param
    else:
        lf = _f32c(language_features.detach())
    a.language_feature = _ptr(lf)
    if out is None and (want_grad or update is None):
        out = torch.empty((L, P, 3), dtype=torch.float32, device=device)
    nbytes = int(lib.lsr_backward_levels_bytes(P, L))
    if scratch is None:
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    elif scratch.dtype != torch.uint8 or scratch.numel() < nbytes:
        raise ValueError(f"levels_step_backward: scratch must be a uint8 tensor of at least {nbytes} bytes")
    if out is not None and (tuple(out.shape) != (L, P, 3) or out.dtype != torch.float32 or not out.is_contiguous()):
        raise ValueError(f"levels_step_backward: out must be a contiguous fp32 ({L}, {P}, 3) tensor")
    a.scratch = _ptr(scratch)
    a.dL_dlanguage_feature = _ptr(out)
    if update is not None:
        tab = update.table()
        keep.append(tab)
        a.update = ctypes.pointer(tab)
        a.update_step_dev = _vp(update.step_dev.data_ptr())
        a.update_skip = _ptr(update.skip)
        a.fill_record = None if update.fill_record is None else _vp(int(update.fill_record))
        a.fill_levels = _ptr(update.fill_levels)
    with _on_device(device):
        _check(lib.lsr_levels_step_backward(ctypes.byref(s), ctypes.byref(a), _stream(device)),
               "lsr_levels_step_backward")
    return out


# LSR_ALL_GRADS=1 (or setting this to True) computes every geometry gradient even when no input
# needs one -- the reference extension's behaviour; kept for comparisons and debugging.
FORCE_GEOMETRY_GRADS = os.environ.get("LSR_ALL_GRADS", "0") == "1"


def geometry_grads_needed(needs_input_grad, geometry_inputs):
    """True if an autograd input among `geometry_inputs` (everything but means2D and the language
    feature) needs a gradient -- torch's ctx.needs_input_grad, as any autograd.Function uses it."""
    return FORCE_GEOMETRY_GRADS or any(needs_input_grad[i] for i in geometry_inputs)


def rasterize_gaussians_backward(rs, means3D, shs, colors_precomp, language_feature, scales, rotations,
                                 cov3D_precomp, radii, grad_color, grad_language, num_rendered, geom, binning,
                                 image, raw=0, shs_rest=None, opacities=None, geometry=True, grad_loss=None,
                                 flags=0, update=None):
    """Native backward: returns the gradient tensors keyed like the reference's inputs (with raw
    flags: w.r.t. the raw parameters; "shs" is then dL/dfeatures_dc and "shs_rest"
    dL/dfeatures_rest).  geometry=False (no geometry input needs a gradient): only "means2D" and
    "language_feature_precomp" are computed, the other entries are None (include/lsr.h).
    grad_loss: dL/d(the fused loss of the forward), a () device tensor, or None.  update: a
    fused_update whose Adam step the backward applies to language_feature (include/lsr.h
    lsr_backward_args.update).  flags: lsr_backward_flags, and BIND_BACKWARD when the forward was made
    in the bound form (forward_bound() at the time of the forward)."""
    lib = load()
    device = means3D.device
    P = int(means3D.shape[0])
    split = shs_rest is not None and shs_rest.numel() > 0
    M_dc = int(shs.shape[1]) if shs is not None and shs.numel() > 0 else 0
    M_rest = int(shs_rest.shape[1]) if split else 0
    M = M_dc + M_rest
    keep: list = []
    s = make_settings(rs, keep)
    # every gradient output is a view of ONE allocation (one caching-allocator call per backward)
    shapes = [("means2D", (P, 3)), ("language_feature_precomp", (P, 3))]
    if geometry:
        shapes += [("colors_precomp", (P, 3)), ("opacities", (P, 1)), ("means3D", (P, 3))]
    if geometry and _ptr(cov3D_precomp) is not None:
        shapes.append(("cov3D_precomp", (P, 6)))
    if geometry and M_dc > 0:
        shapes.append(("shs", (P, M_dc, 3)))
    if geometry and split:
        shapes.append(("shs_rest", (P, M_rest, 3)))
    if geometry and _ptr(scales) is not None:
        shapes.append(("scales", (P, 3)))
    if geometry and _ptr(rotations) is not None:
        shapes.append(("rotations", (P, 4)))
    sizes = [math.prod(sh) for _, sh in shapes]
    aligned = [(n + 63) // 64 * 64 for n in sizes]  # 256-B aligned views (vector loads/stores)
    flat = torch.empty((max(sum(aligned), 1),), dtype=torch.float32, device=device)
    g = dict.fromkeys(("means2D", "colors_precomp", "language_feature_precomp", "opacities", "means3D",
                       "cov3D_precomp", "shs", "shs_rest", "scales", "rotations"))
    off = 0
    for (name, sh), n, na in zip(shapes, sizes, aligned):
        g[name] = flat[off:off + n].view(sh)
        off += na
    if P == 0:
        if update is not None and update.defer:
            update.pending = (None, None, [], torch.empty((0,), dtype=torch.float32, device=device), device)
            update.used = True
        return {k: (v.zero_() if v is not None else None) for k, v in g.items()}
    a = LsrBackwardArgs()
    a.P = P
    a.M = M
    a.num_rendered = int(num_rendered)
    a.means3D = _ptr(means3D)
    a.shs = _ptr(shs)
    a.colors_precomp = _ptr(colors_precomp)
    a.language_feature = _ptr(language_feature)
    a.opacities = _ptr(opacities)
    a.raw = int(raw)
    a.flags = int(flags)
    if split:
        a.shs_rest = _ptr(shs_rest)
        a.dL_dsh_rest = _ptr(g["shs_rest"])
    a.scales = _ptr(scales)
    a.rotations = _ptr(rotations)
    a.cov3D_precomp = _ptr(cov3D_precomp)
    a.radii = _ptr(radii)
    gc = _f32c(grad_color.detach()) if grad_color is not None else None  # None: zero colour gradient
    a.dL_dout_color = _ptr(gc)
    gl = None
    if grad_language is not None:
        gl = _f32c(grad_language.detach())
        a.dL_dout_language_feature = _ptr(gl)
    gls = None
    if grad_loss is not None:
        gls = _f32c(grad_loss.detach().reshape(1))
        a.dL_dloss = _ptr(gls)
    a.geom_buffer = _ptr(geom)
    a.binning_buffer = _ptr(binning)
    a.image_buffer = _ptr(image)
    a.dL_dmeans2D = _ptr(g["means2D"])
    a.dL_dcolors = _ptr(g["colors_precomp"])
    a.dL_dlanguage_feature = _ptr(g["language_feature_precomp"])
    a.dL_dopacity = _ptr(g["opacities"])
    a.dL_dmeans3D = _ptr(g["means3D"])
    a.dL_dcov3D = _ptr(g["cov3D_precomp"])
    a.dL_dsh = _ptr(g["shs"])
    a.dL_dscales = _ptr(g["scales"])
    a.dL_drotations = _ptr(g["rotations"])
    if update is not None:
        tab = update.table()
        keep.append(tab)
        a.update = ctypes.pointer(tab)
        a.update_step_dev = ctypes.c_void_p(update.optimizer._step_dev.data_ptr())
        a.update_skip = _ptr(update.skip)
        a.fill_record = None if update.fill is None else ctypes.c_void_p(int(update.fill))
        update.used = True
        if update.defer:
            a.flags |= BWD_DEFER_TAIL
        if update.fill is not None and update.fill_plane:
            a.flags |= BIND_FILL_PLANE
    alloc = _Allocator(device)
    with _on_device(device), alloc:
        _check(lib.lsr_backward(ctypes.byref(s), ctypes.byref(a), _ALLOC_CB, None, _stream(device)), "lsr_backward")
    if update is not None and update.defer:
        # the records' language partials and the skip word: the first 3 P + 1 floats of grad_records
        off = state_layout(P, int(rs.image_width), int(rs.image_height), int(num_rendered))["grad_records"]
        part = geom[off:off + 4 * (3 * P + 1)].view(torch.float32)
        # every tensor the deferred launch's pointers reach stays alive with it
        keep += [flat, geom, binning, image, radii, language_feature, update.skip, gl, gls, gc, means3D]
        update.pending = (s, a, keep, part, device)
    return g


def densification_stats(radii, dmeans2D, max_radii2D=None, xyz_gradient_accum=None, denom=None):
    """train.py:125-126 in one kernel (include/lsr.h lsr_densification_stats), in place: for radii > 0,
    max_radii2D = max(max_radii2D, radii), xyz_gradient_accum += ||dmeans2D[:, :2]||, denom += 1."""
    lib = load()
    P = int(radii.shape[0])
    outs = []
    for t, shape in ((max_radii2D, (P,)), (xyz_gradient_accum, (P, 1)), (denom, (P, 1))):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != P):
            raise ValueError(f"densification_stats: expected a contiguous fp32 tensor of {shape}")
        outs.append(_ptr(t))
    if radii.dtype != torch.int32 or not radii.is_contiguous():
        raise ValueError("densification_stats: radii must be a contiguous int32 tensor")
    g = _f32c(dmeans2D.detach())
    if tuple(g.shape) != (P, 3):
        raise ValueError("densification_stats: dmeans2D must be (P, 3)")
    with _on_device(radii.device):
        _check(lib.lsr_densification_stats(P, _ptr(radii), _ptr(g), *outs, _stream(radii.device)),
               "lsr_densification_stats")


def fill_language(language_feature: torch.Tensor, raw: int, radii: torch.Tensor, record_ptr: int, plane: bool = False):
    """The language slots of a geometry-phase forward's render records from the parameter, on the
    current stream (include/lsr.h lsr_fill_language); plane: record_ptr is a bound set's plane
    (lsr_fill_language_plane)."""
    P = int(radii.shape[0])
    lf = _f32c(language_feature.detach())
    if tuple(lf.shape) != (P, 3) or radii.dtype != torch.int32 or not radii.is_contiguous():
        raise ValueError("fill_language: a (P, 3) feature and the (P,) int32 radii of the same forward")
    with _on_device(lf.device):
        fn = load().lsr_fill_language_plane if plane else load().lsr_fill_language
        _check(fn(P, _ptr(lf), int(raw), _ptr(radii), ctypes.c_void_p(int(record_ptr)), _stream(lf.device)),
               "lsr_fill_language")


def view_pack_bytes(P: int, W: int, H: int, num_rendered: int) -> int:
    """Bytes of a view pack (include/lsr.h lsr_view_pack_bytes)."""
    return int(load().lsr_view_pack_bytes(int(P), int(W), int(H), int(num_rendered)))


def has_view_plan() -> bool:
    """The library keeps a view's walk plan in packs of view_plan_pack_bytes (include/lsr.h)."""
    lib = load()
    return all(hasattr(lib, n) for n in OPTIONAL_PLAN)


def view_plan_pack_bytes(P: int, W: int, H: int, num_rendered: int) -> int:
    """Bytes of a view pack with room for the walk plan (include/lsr.h lsr_view_plan_pack_bytes)."""
    return int(load().lsr_view_plan_pack_bytes(int(P), int(W), int(H), int(num_rendered)))


def view_plan_layout(P: int, W: int, H: int, capacity_rendered: int, num_rendered: int) -> Dict[str, int]:
    """Byte offsets of the walk plan's segments in a pack and of the set's arrays they are saved from
    (include/lsr.h lsr_view_plan_layout)."""
    lay = LsrViewPlanOffsets()
    _check(load().lsr_view_plan_layout(int(P), int(W), int(H), int(capacity_rendered), int(num_rendered),
                                       ctypes.byref(lay)), "lsr_view_plan_layout")
    return {name: int(getattr(lay, name)) for name, _ in LsrViewPlanOffsets._fields_}


def view_args(buffers: "static_buffers", num_rendered: int, pack: torch.Tensor) -> LsrViewArgs:
    """lsr_view_args of one static_buffers set whose geometry-phase forward has run (its geometry_call
    record: sizes, capacities, flags) and one pack tensor (uint8, at least view_pack_bytes)."""
    call = buffers.geometry_call
    a = LsrViewArgs()
    a.P, a.width, a.height = call["P"], call["W"], call["H"]
    a.flags, a.fused_loss = call["flags"], call["fused_loss"]
    a.capacity_rendered, a.capacity_entries = call["rendered"], call["entries"]
    a.num_rendered = int(num_rendered)
    a.geom = buffers.tensors[("scratch", LSR_BUF_GEOM)].data_ptr()
    a.image = buffers.tensors[("scratch", LSR_BUF_IMAGE)].data_ptr()
    a.binning = buffers.tensors[("scratch", LSR_BUF_BINNING)].data_ptr()
    a.radii = buffers.tensors[("out", "radii")].data_ptr()
    a.pack = pack.data_ptr()
    a.pack_bytes = int(pack.numel())
    a.overflow = call["overflow"].data_ptr()
    return a


def view_counts(W: int, H: int, image: torch.Tensor, host: torch.Tensor, stream: "torch.cuda.Stream"):
    """The set's eight counter slots (image: its LSR_BUF_IMAGE buffer) into `host`, a pinned int32 tensor
    of 8, by a kernel on `stream` (include/lsr.h lsr_view_counts)."""
    if not host.is_pinned() or host.dtype != torch.int32 or host.numel() < 8:
        raise ValueError("view_counts: host must be a pinned int32 tensor of at least 8 elements")
    with _on_device(stream.device):
        _check(load().lsr_view_counts(int(W), int(H), _vp(image.data_ptr()), _vp(host.data_ptr()),
                                      _vp(stream.cuda_stream)), "lsr_view_counts")


def view_save(args: LsrViewArgs, stream: "torch.cuda.Stream"):
    """The set's kept geometry into the pack, enqueued on `stream` (include/lsr.h lsr_view_save)."""
    with _on_device(stream.device):
        _check(load().lsr_view_save(ctypes.byref(args), _vp(stream.cuda_stream)), "lsr_view_save")


def view_restore(args: LsrViewArgs, stream: "torch.cuda.Stream"):
    """The pack back into the set in place of its geometry call, enqueued on `stream` (lsr_view_restore)."""
    with _on_device(stream.device):
        _check(load().lsr_view_restore(ctypes.byref(args), _vp(stream.cuda_stream)), "lsr_view_restore")


def has_view_bind() -> bool:
    """The library has the bound form's entry points (include/lsr.h lsr_view_bind)."""
    lib = load()
    return all(hasattr(lib, n) for n in OPTIONAL)


def view_bind_layout(P: int, W: int, H: int) -> Dict[str, int]:
    """Byte offsets of a set's plane and table in its geometry buffer (lsr_view_bind_layout)."""
    plane, table = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(load().lsr_view_bind_layout(int(P), int(W), int(H), ctypes.byref(plane), ctypes.byref(table)),
           "lsr_view_bind_layout")
    return {"plane": int(plane.value), "table": int(table.value)}


def view_bind(args: LsrViewArgs, stream: "torch.cuda.Stream", clamped: bool = False):
    """The set bound to args' pack (args.pack None: to its own arrays) in place of its geometry call or a
    restore, enqueued on `stream` (include/lsr.h lsr_view_bind)."""
    with _on_device(stream.device):
        _check(load().lsr_view_bind(ctypes.byref(args), BIND_CLAMPED if clamped else 0, _vp(stream.cuda_stream)),
               "lsr_view_bind")


def mark_visible(means3D, viewmatrix, projmatrix):
    lib = load()
    device = means3D.device
    P = int(means3D.shape[0])
    vis = torch.zeros((P,), dtype=torch.uint8, device=device)
    m = _f32c(means3D.detach())
    v = _f32c(viewmatrix.detach())
    p = _f32c(projmatrix.detach())
    with _on_device(device):
        _check(lib.lsr_mark_visible(P, _ptr(m), _ptr(v), _ptr(p), _ptr(vis), _stream(device)), "lsr_mark_visible")
    return vis.bool()


def state_layout(P: int, W: int, H: int, num_rendered: int) -> Dict[str, int]:
    lay = LsrStateLayout()
    _check(load().lsr_state_layout_of(P, W, H, num_rendered, ctypes.byref(lay)), "lsr_state_layout_of")
    return {name: int(getattr(lay, name)) for name, _ in LsrStateLayout._fields_}


def profile_enable(on: bool = True, stages=None, every: int = 1):
    """Start (clearing) / stop the per-stage HIP-event profiler; `stages` restricts it to those
    stage names (lsr_profile_select), `every` > 1 records only every every-th selected launch
    (lsr_profile_sample)."""
    lib = load()
    lib.lsr_profile_select(",".join(stages).encode() if stages else None)
    _check(lib.lsr_profile_sample(int(every)), "lsr_profile_sample")
    lib.lsr_profile_enable(1 if on else 0)


def profile_report() -> Dict[str, Dict[str, float]]:
    """{stage: {"launches": n, "total_ms": t, "avg_ms": t / n}} (synchronises recorded events)."""
    lib = load()
    n = lib.lsr_profile_report(None, 0)
    arr = (LsrKernelStat * max(n, 1))()
    n = lib.lsr_profile_report(arr, n)
    out = {}
    for i in range(n):
        k = arr[i].name.decode()
        out[k] = {"launches": int(arr[i].launches), "total_ms": float(arr[i].total_ms),
                  "avg_ms": float(arr[i].total_ms) / max(int(arr[i].launches), 1)}
    return out


def debug_render_stats():
    """Counters of the LSR_RENDER_STATS=1 backward (include/lsr.h lsr_debug_render_stats); clears them."""
    arr = (ctypes.c_uint64 * 73)()
    _check(load().lsr_debug_render_stats(arr, 73), "lsr_debug_render_stats")
    v = list(arr)
    return {"entries": v[0], "power_hit": v[1], "alpha_hit": v[2], "lanes_hit": v[3], "barrier_slots": v[4],
            "batches": v[6], "hist": v[8:8 + 65]}


def debug_knn_grid(box, N):
    """The search grid lsr_dist_cuda2 sizes for N points in the bounding box (min x, y, z, max x, y, z),
    evaluated on the host (include/lsr.h lsr_debug_knn_grid): {"origin": (x0, y0, z0), "h", "inv_h",
    "dims": (nx, ny, nz)}."""
    b = (ctypes.c_float * 6)(*box)
    o = (ctypes.c_float * 5)()
    d = (ctypes.c_int32 * 3)()
    _check(load().lsr_debug_knn_grid(b, N, o, d), "lsr_debug_knn_grid")
    return {"origin": tuple(o[:3]), "h": o[3], "inv_h": o[4], "dims": tuple(d)}


def debug_render_timeline(kernel, n):
    """Per-workgroup timeline of the LSR_RENDER_STATS=1 render kernels (kernel 0 forward, 1 backward;
    include/lsr.h lsr_debug_render_timeline): for workgroups < n, dicts with start, end, tile,
    slot and (forward) the load / compact / walk ticks, the batch count, the first batch's load ticks and its milestones (ticks after the start: begin,
    ranges loaded, first barrier, ids loaded, records gathered, load phase done)."""
    W = 11
    arr = (ctypes.c_uint32 * (W * n))()
    _check(load().lsr_debug_render_timeline(kernel, arr, n), "lsr_debug_render_timeline")
    v = list(arr)
    out = []
    for i in range(n):
        r = v[W * i:W * i + W]
        out.append({"start": r[0], "end": r[1], "tile": r[2] if r[2] < 2 ** 31 else r[2] - 2 ** 32, "slot": r[3],
                    "load": r[4], "compact": r[5], "walk": r[6], "batches": r[7] & 0xFFFF,
                    "first_load": r[7] >> 16,
                    "first_marks": [r[8] & 0xFFFF, r[8] >> 16, r[9] & 0xFFFF, r[9] >> 16, r[10] & 0xFFFF, r[10] >> 16]})
    return out

