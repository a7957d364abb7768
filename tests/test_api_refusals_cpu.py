"""The refusals of the native API layer, pinned byte for byte: for every case below the status code and the
complete lsr_last_error() text equal tests/golden/api_refusals.json, which tests/golden/make_api_refusals.py
recorded from the library as it was before the layer's checks were factored into shared helpers.  The
cases are those of test_levels_cpu, test_levels_train_cpu, test_levels_graph_cpu, test_view_cache_cpu,
test_view_bind_cpu and test_native_abi's lsr_forward / lsr_backward / lsr_language_tail ones, the remaining
checks of lsr_forward and lsr_backward, and per shared validator cases with two faults, which pin the order
of the checks: the earlier one answers.  Every call is refused before any device work (dummy pointers,
never dereferenced), so no GPU is needed."""
import ctypes
import json
import os

from langsplat_amd import _native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_refusals.json")
D = 0x10000  # a non-NULL, 16-byte aligned "pointer" no refusal path reads
FUSED = ("out_language_feature", "loss_target", "loss_mask", "dL_dloss")
GEOMETRY, COMPOSITE, COMPOSITE_FILLED = (_native.forward_phase.GEOMETRY, _native.forward_phase.COMPOSITE,
                                         _native.forward_phase.COMPOSITE_FILLED)
NO_BWD = _native.FWD_NO_BACKWARD
SHORT = "one byte short"


def _settings(over):
    """lsr_settings for an 8 x 8 image; over: field overrides, or None for a NULL settings pointer."""
    if over is None:
        return None
    s = _native.LsrSettings()
    s.image_height, s.image_width, s.tanfovx, s.tanfovy, s.sh_degree, s.include_feature = 8, 8, 0.5, 0.5, 0, 1
    s.bg = s.viewmatrix = s.projmatrix = s.campos = D
    for k, v in over.items():
        setattr(s, k, v)
    return ctypes.byref(s)


def _fill_forward(a, kw):
    a.P, a.M = 4, 1
    a.means3D = a.shs = a.opacities = a.scales = a.rotations = a.language_feature = D
    a.out_color = a.out_language_feature = a.radii = D
    for k, v in kw.items():
        setattr(a, k, v)


def _forward(lib, settings={}, args=True, **kw):
    a = _native.LsrForwardArgs()
    _fill_forward(a, kw)
    nr = ctypes.c_int64(0)
    return lib.lsr_forward(_settings(settings), ctypes.byref(a) if args else None, _native._ALLOC_CB, None, None,
                           ctypes.byref(nr))


def _fill_levels(la, levels, more, kw):
    own = ("reserved", "more_language_feature", "more_out_language_feature")
    _fill_forward(la.fwd, dict({"flags": NO_BWD}, **{k: v for k, v in kw.items() if k not in own}))
    la.levels = levels
    if more:
        la.more_language_feature = la.more_out_language_feature = D
    for k in own:
        if k in kw:
            setattr(la, k, kw[k])


def _forward_levels(lib, settings={}, args=True, levels=3, more=True, **kw):
    la = _native.LsrForwardLevelsArgs()
    _fill_levels(la, levels, more, kw)
    nr = ctypes.c_int64(0)
    return lib.lsr_forward_levels(_settings(settings), ctypes.byref(la) if args else None, _native._ALLOC_CB, None,
                                  None, ctypes.byref(nr))


def _levels_step_forward(lib, settings={}, args=True, levels=3, more=True, outer_reserved=0, **kw):
    sa = _native.LsrLevelsStepForwardArgs()
    sa.reserved = outer_reserved
    _fill_levels(sa.levels, levels, more, dict(dict(capacity_rendered=64, capacity_entries=64, overflow=D), **kw))
    nr = ctypes.c_int64(0)
    return lib.lsr_levels_step_forward(_settings(settings), ctypes.byref(sa) if args else None, _native._ALLOC_CB,
                                       None, None, ctypes.byref(nr))


def _fill_levels_backward(a, num_rendered, kw):
    a.P, a.levels, a.num_rendered = 4, 3, num_rendered
    for name in ("geom_buffer", "binning_buffer", "image_buffer", "radii", "language_feature",
                 "dL_dout_language_feature", "scratch", "dL_dlanguage_feature"):
        setattr(a, name, D)
    for k, v in kw.items():
        setattr(a, k, v)


def _backward_levels(lib, settings={}, args=True, **kw):
    a = _native.LsrBackwardLevelsArgs()
    _fill_levels_backward(a, 10, kw)
    return lib.lsr_backward_levels(_settings(settings), ctypes.byref(a) if args else None, None)


def _levels_step_backward(lib, settings={}, args=True, update=None, **kw):
    """update: None, or overrides of the lsr_adam_tensor of a fused update (n, param, exp_avg, exp_avg_sq)."""
    a = _native.LsrLevelsStepBackwardArgs()
    keep = None
    if update is not None:
        u = dict(dict(n=3 * 3 * 4, param=D, exp_avg=D, exp_avg_sq=D), **update)
        keep = _native.LsrAdamTensor(u["n"], u["param"], None, u["exp_avg"], u["exp_avg_sq"], 0.0, 0.9, 0.999, 1e-15, 0)
        kw = dict(dict(update=ctypes.pointer(keep), raw=_native.RAW_LANGUAGE, update_step_dev=D), **kw)
    _fill_levels_backward(a, 64, kw)
    return lib.lsr_levels_step_backward(_settings(settings), ctypes.byref(a) if args else None, None)


def _fill_backward(a, update, kw):
    """The language-only backward of a raw feature, with update its fused Adam step (overrides of the tensor)."""
    a.P, a.M, a.num_rendered = 4, 1, 16
    a.means3D = a.shs = a.opacities = a.scales = a.rotations = a.radii = a.language_feature = D
    a.geom_buffer = a.binning_buffer = a.image_buffer = a.dL_dmeans2D = a.dL_dlanguage_feature = D
    a.raw = _native.RAW_LANGUAGE
    keep = None
    if update is not None:
        u = dict(dict(n=3 * 4, param=D, exp_avg=2 * D, exp_avg_sq=3 * D), **update)
        keep = _native.LsrAdamTensor(u["n"], u["param"], None, u["exp_avg"], u["exp_avg_sq"], 0.01, 0.9, 0.999, 1e-15, 0)
        a.update = ctypes.pointer(keep)
        a.update_step_dev = D
    for k, v in kw.items():
        setattr(a, k, v)
    return keep


def _backward(lib, settings={}, args=True, update=None, geometry=False, **kw):
    a = _native.LsrBackwardArgs()
    if geometry:
        kw = dict({n: D for n in ("dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dsh", "dL_dscales",
                                  "dL_drotations")}, **kw)
    keep = _fill_backward(a, update, kw)  # noqa: F841 (the tensor lives until the call returns)
    return lib.lsr_backward(_settings(settings), ctypes.byref(a) if args else None, _native._ALLOC_CB, None, None)


def _language_tail(lib, settings={}, args=True, update={}, **kw):
    a = _native.LsrBackwardArgs()
    keep = _fill_backward(a, update, kw)  # noqa: F841 (the tensor lives until the call returns)
    return lib.lsr_language_tail(_settings(settings), ctypes.byref(a) if args else None, None)


def _view_args(lib, kw):
    """A valid hit (a pack of exactly lsr_view_pack_bytes); pack_bytes=SHORT: one byte less."""
    a = _native.LsrViewArgs()
    a.P, a.width, a.height = 100, 70, 50
    a.capacity_rendered, a.capacity_entries, a.num_rendered = 5000, 4000, 1234
    a.geom = a.image = a.binning = a.radii = a.pack = D
    a.pack_bytes = int(lib.lsr_view_pack_bytes(100, 70, 50, 1234))
    for k, v in kw.items():
        setattr(a, k, a.pack_bytes - 1 if v is SHORT else v)
    return a


def _view_save(lib, args=True, **kw):
    return lib.lsr_view_save(ctypes.byref(_view_args(lib, kw)) if args else None, None)


def _view_restore(lib, args=True, **kw):
    return lib.lsr_view_restore(ctypes.byref(_view_args(lib, kw)) if args else None, None)


def _view_bind(lib, args=True, bind_flags=0, **kw):
    return lib.lsr_view_bind(ctypes.byref(_view_args(lib, kw)) if args else None, bind_flags, None)


def _cases():
    """(entry point's caller, its keyword arguments): every refusal, then the two-fault cases."""
    c = []
    # lsr_forward: every check of the forward's arguments, in their order
    c += [(_forward, kw) for kw in [
        dict(settings=None), dict(args=False), dict(P=-1), dict(settings=dict(image_width=0)),
        dict(settings=dict(image_height=65535 * 16 + 1)), dict(settings=dict(sh_degree=4)), dict(out_color=None),
        dict(radii=None), dict(shs=None), dict(colors_precomp=D), dict(cov3D_precomp=D), dict(scales=None), dict(M=0),
        dict(settings=dict(bg=None)), dict(raw=16), dict(flags=8), dict(flags=_native.BIND_FORWARD),
        dict(shs_rest=D), dict(capacity_rendered=-1), dict(capacity_rendered=16), dict(capacity_entries=1 << 32),
        dict(phase=GEOMETRY), dict(phase=4, capacity_rendered=16, capacity_entries=16), dict(phase=COMPOSITE_FILLED),
        dict(phase=COMPOSITE, capacity_rendered=16, capacity_entries=16, language_ready=D), dict(phase=-1),
        dict(out_loss=D), dict(out_loss=D, loss_target=D, loss_mask=D, settings=dict(include_feature=0)),
        dict(out_loss=D, loss_target=D, loss_mask=D, language_feature=None),
        # two faults: the earlier check answers
        dict(P=-1, settings=dict(sh_degree=4)), dict(flags=8, phase=GEOMETRY), dict(raw=16, flags=8),
        dict(shs_rest=D, capacity_rendered=-1), dict(phase=GEOMETRY, out_loss=D), dict(M=0, out_color=None)]]
    # lsr_forward_levels (test_levels_cpu), and what the forward refuses behind its own checks
    c += [(_forward_levels, kw) for kw in [
        dict(settings=None), dict(args=False), dict(levels=0), dict(levels=5), dict(levels=-1), dict(reserved=1),
        dict(settings=dict(include_feature=0)), dict(flags=0), dict(flags=_native.FWD_ZERO_GRAD_RECORDS),
        dict(flags=NO_BWD | _native.FWD_NO_COLOR_GRAD), dict(loss_target=D), dict(loss_mask=D), dict(out_loss=D),
        dict(language_ready=D), dict(phase=GEOMETRY), dict(phase=COMPOSITE, capacity_rendered=16, capacity_entries=16),
        dict(capacity_rendered=16, capacity_entries=16), dict(language_feature=None), dict(more_language_feature=None),
        dict(more_out_language_feature=None), dict(more=False), dict(M=0), dict(levels=1, more=False, P=-1),
        dict(settings=dict(sh_degree=4)),
        dict(levels=0, reserved=1), dict(reserved=1, flags=0), dict(flags=0, loss_target=D),
        dict(language_ready=D, phase=GEOMETRY), dict(phase=GEOMETRY, capacity_rendered=16),
        dict(capacity_rendered=16, language_feature=None), dict(language_feature=None, more_language_feature=None),
        dict(more_out_language_feature=None, M=0)]]
    # lsr_levels_step_forward (test_levels_graph_cpu)
    c += [(_levels_step_forward, kw) for kw in [
        dict(settings=None), dict(args=False), dict(levels=0), dict(levels=5), dict(reserved=1),
        dict(outer_reserved=1), dict(settings=dict(include_feature=0)), dict(flags=0),
        dict(flags=NO_BWD | _native.FWD_ZERO_GRAD_RECORDS), dict(loss_target=D), dict(loss_mask=D), dict(out_loss=D),
        dict(language_ready=D), dict(capacity_rendered=0), dict(capacity_rendered=-1), dict(capacity_entries=0),
        dict(overflow=None), dict(phase=GEOMETRY), dict(phase=4), dict(phase=-1), dict(language_feature=None),
        dict(more_language_feature=None), dict(more_out_language_feature=None), dict(more=False), dict(M=0),
        dict(flags=NO_BWD | _native.BIND_FORWARD),
        dict(levels=5, outer_reserved=1), dict(outer_reserved=1, flags=0), dict(out_loss=D, language_ready=D),
        dict(language_ready=D, capacity_rendered=0), dict(capacity_entries=0, overflow=None),
        dict(overflow=None, phase=GEOMETRY), dict(phase=4, language_feature=None),
        dict(language_feature=None, more_out_language_feature=None), dict(more_language_feature=None, M=0)]]
    # lsr_backward_levels (test_levels_train_cpu) and lsr_levels_step_backward (test_levels_graph_cpu)
    shared = [
        dict(settings=None), dict(args=False), dict(levels=0), dict(levels=5), dict(levels=-1), dict(reserved=1),
        dict(P=-1), dict(num_rendered=-1), dict(settings=dict(include_feature=0)),
        dict(settings=dict(image_width=0)), dict(settings=dict(image_height=-1)), dict(geom_buffer=None),
        dict(binning_buffer=None), dict(image_buffer=None), dict(radii=None), dict(scratch=None),
        dict(dL_dlanguage_feature=None), dict(raw=_native.RAW_LANGUAGE, language_feature=None),
        dict(dL_dout_language_feature=None), dict(P=0, dL_dout_language_feature=None)]
    shared += [dict({n: D for n in FUSED if n != miss}) for miss in FUSED]
    shared += [dict({n: D}, dL_dout_language_feature=None) for n in FUSED]
    shared += [  # two faults
        dict(settings=None, args=False), dict(levels=0, reserved=1), dict(reserved=1, P=-1), dict(P=-1, num_rendered=-1),
        dict(num_rendered=-1, settings=dict(include_feature=0)), dict(settings=dict(include_feature=0, image_width=0)),
        dict(settings=dict(image_width=0), geom_buffer=None), dict(num_rendered=0, geom_buffer=None),
        dict(geom_buffer=None, binning_buffer=None), dict(image_buffer=None, radii=None), dict(radii=None, scratch=None),
        dict(scratch=None, dL_dlanguage_feature=None),
        dict(dL_dlanguage_feature=None, raw=_native.RAW_LANGUAGE, language_feature=None),
        dict(raw=_native.RAW_LANGUAGE, language_feature=None, loss_target=D), dict(loss_target=D, geom_buffer=None),
        dict(P=0, geom_buffer=None, loss_mask=D)]
    c += [(_backward_levels, kw) for kw in shared]
    c += [(_levels_step_backward, kw) for kw in shared + [
        dict(reserved2=1), dict(num_rendered=0), dict(update={}, raw=0), dict(update=dict(param=2 * D)), dict(update=dict(n=3 * 4)),
        dict(update=dict(n=3 * 3 * 4 + 1)), dict(update=dict(exp_avg=None)), dict(update=dict(exp_avg_sq=None)),
        dict(update={}, update_step_dev=None), dict(update={}, fill_record=D), dict(update={}, fill_levels=D),
        dict(fill_record=D), dict(fill_levels=D), dict(update_step_dev=D), dict(update_skip=D),
        dict(update=dict(n=1), dL_dlanguage_feature=None), dict(levels=0, reserved2=1), dict(reserved2=1, P=-1),
        dict(update={}, raw=0, dL_dout_language_feature=None), dict(update=dict(n=1), scratch=None),
        dict(update=dict(n=1, param=2 * D)), dict(fill_record=D, loss_target=D)]]
    # lsr_backward and lsr_language_tail (test_native_abi, test_view_bind_cpu)
    c += [(_backward, kw) for kw in [
        dict(settings=None), dict(args=False), dict(P=-1), dict(settings=dict(image_width=0)),
        dict(dL_dcolors=D), dict(geometry=True, dL_dsh=None), dict(geometry=True, cov3D_precomp=D), dict(raw=16),
        dict(flags=64), dict(flags=_native.BIND_FILL_PLANE), dict(flags=_native.BWD_DEFER_TAIL),
        dict(geometry=True, shs_rest=D), dict(raw=_native.RAW_LANGUAGE | _native.RAW_OPACITY, opacities=None),
        dict(update={}, geometry=True), dict(update={}, raw=0), dict(update=dict(param=2 * D)),
        dict(update={}, dL_dout_color=D), dict(update={}, update_step_dev=None), dict(update=dict(n=3)),
        dict(update=dict(exp_avg=None)), dict(update={}, settings=dict(include_feature=0)), dict(fill_record=D),
        dict(update_step_dev=D), dict(update_skip=D), dict(update={}, geometry=True, flags=_native.BWD_DEFER_TAIL),
        dict(geom_buffer=None), dict(radii=None),
        dict(P=-1, raw=16), dict(dL_dcolors=D, raw=16), dict(raw=16, flags=64), dict(flags=64 | _native.BIND_FILL_PLANE),
        dict(flags=_native.BIND_FILL_PLANE | _native.BWD_DEFER_TAIL), dict(flags=_native.BWD_DEFER_TAIL, fill_record=D),
        dict(fill_record=D, geom_buffer=None)]]
    c += [(_language_tail, kw) for kw in [
        dict(settings=None), dict(args=False), dict(P=-1), dict(update=None), dict(raw=0),
        dict(dL_dlanguage_feature=None), dict(update=dict(param=2 * D)), dict(update=dict(n=3)),
        dict(update=dict(exp_avg_sq=None)), dict(update_step_dev=None), dict(geom_buffer=None), dict(radii=None),
        dict(fill_record=D + 8), dict(P=-1, update=None), dict(raw=0, geom_buffer=None),
        dict(geom_buffer=None, fill_record=D + 8)]]
    # lsr_view_save / lsr_view_restore (test_view_cache_cpu) and lsr_view_bind (test_view_bind_cpu)
    view = [
        dict(args=False), dict(P=0), dict(P=-3), dict(width=0), dict(height=-1), dict(width=65535 * 16 + 1),
        dict(capacity_rendered=0), dict(capacity_entries=0), dict(capacity_rendered=1 << 32), dict(num_rendered=-1),
        dict(num_rendered=5001), dict(geom=None), dict(image=None), dict(binning=None), dict(radii=None),
        dict(pack_bytes=SHORT), dict(pack_bytes=0), dict(pack=D + 8), dict(geom=D + 4), dict(radii=D + 2),
        dict(flags=8), dict(flags=_native.BIND_FORWARD), dict(reserved=1),
        # two faults; the copies look at num_rendered before the buffers, lsr_view_bind after them
        # (without a pack lsr_view_bind looks at neither num_rendered nor pack_bytes: a miss, refused here for its flag)
        dict(P=0, capacity_rendered=0), dict(capacity_entries=0, num_rendered=-1), dict(num_rendered=-1, geom=None),
        dict(geom=None, pack_bytes=0), dict(geom=None, pack=None, pack_bytes=0), dict(pack_bytes=0, geom=D + 4),
        dict(radii=D + 2, flags=8), dict(pack=None, pack_bytes=0, flags=8),
        dict(pack=None, num_rendered=-1, pack_bytes=0, flags=8)]
    for fn in (_view_save, _view_restore, _view_bind):
        c += [(fn, kw) for kw in view]
    for fn in (_view_save, _view_restore):  # the copies need the pack
        c += [(fn, kw) for kw in [dict(pack=None), dict(num_rendered=5001, pack=None), dict(pack=None, pack_bytes=0)]]
    c += [(_view_bind, kw) for kw in [dict(bind_flags=2), dict(bind_flags=2, P=0), dict(args=False, bind_flags=2)]]
    return c


def _show(v):
    if isinstance(v, dict):
        return "{" + ",".join(f"{k}={_show(x)}" for k, x in sorted(v.items())) + "}"
    return hex(v) if isinstance(v, int) and not isinstance(v, bool) and v >= D else repr(v)


def case_id(fn, kw):
    return fn.__name__.lstrip("_") + "(" + ",".join(f"{k}={_show(v)}" for k, v in sorted(kw.items())) + ")"


def run_cases(lib):
    """{case id: {"code", "message"}} of every case, with the library `lib` (_native.load's)."""
    out = {}
    for fn, kw in _cases():
        key = case_id(fn, kw)
        assert key not in out, key
        rc = fn(lib, **kw)
        out[key] = dict(code=int(rc), message=lib.lsr_last_error().decode())
    return out


def test_every_refusal_is_byte_for_byte_the_recorded_one():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = run_cases(_native.load())
    assert sorted(got) == sorted(want)  # the fixture was generated from these cases
    assert len(want) > 300 and all(v["code"] == 1 and v["message"] for v in want.values())  # LSR_ERR_INVALID, each one
    for key in want:
        assert got[key] == want[key], key
