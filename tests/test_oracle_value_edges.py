"""The oracle at the value edges of the blend and of the activations, against the independent
float64 dense-autograd restatement (oracle/torch_ref.py).  CPU only.

Every other scene of the suite comes from make_gaussians, whose opacity logits, f_dc entries,
quaternions and language vectors almost never reach the values at which the blend changes
behaviour: not one of those scenes holds a blend with o G > 0.99 (alpha clamped, straight-through
gradient, T recovered by a division by 0.01), an opacity of exactly 1 or 0 or under 1/255, a zero
quaternion or a zero language vector, and only a handful of SH channels clamped at 0.
tests/scenes.py edge_gaussians puts seeded subsets of the raw parameters on those values, and
blend_census counts, from the oracle's own state, what a scene reaches; every test asserts the
minimums of scenes.EDGE_MINIMUMS first (conditions, not measurements), so a scene cannot silently
stop reaching an edge.  Census of the committed scenes (scenes.EDGE_SCENES):

    scene                         A        B        C
    blends                    96886    75448   173292
    saturated blends            163      151      115
      Gaussians / tiles       5 / 9    5 / 7    6 / 7
    blends after a saturated    508      354     1595
    clamped SH channels         143      128      186
    clamped + unclamped rows     95       79      127
    o == 1 / == 0 / < 1/255  18/16/16 15/14/14  21/11/5
    zero quaternion / language 10/13    12/-     14/8
    pixels not terminated      2199     1930     5823   (of 6144, 5673, 6144)

Tolerances are those of tests/test_oracle_render.py: radii and contributor counts equal, images
within 2e-5, every gradient within 2e-4 of its tensor's maximum.  Measured when the scenes were
chosen: images within 4.2e-7, gradients within 1.6e-6 (the hand-derived backward holds them with two
orders of margin).  Sensitivity, in a scratch copy of the oracle: with the clamp made
non-straight-through (d alpha = 0 where o G > 0.99) the backward test fails on all three scenes
(means3D off by 3e-3 .. 1.3e-2) while tests/test_oracle_render.py and tests/test_oracle_cameras.py
still pass; without the clamped-colour mask it fails on all three (shs off by up to 1.3).  test_gpu_value_edges.py runs the kernels on the same scenes against this oracle.
"""
import numpy as np
import pytest
import torch

from oracle import oracle, torch_ref
from tests.scenes import (EDGE_SCENES, assert_reaches_edges, blend_census, edge_case, grad_seed, scene)


@pytest.mark.parametrize("name", sorted(EDGE_SCENES))
def test_scene_reaches_the_edges(name):
    c = edge_case(name)
    assert_reaches_edges(c.census, c.include_feature)
    # the saturated logits activate to exactly 1 and 0, the log-scale -100 to exactly 0
    o, raw = c.inp["opacities"].numpy().reshape(-1), c.g.opacity.numpy().reshape(-1)
    assert (raw == 100.0).sum() >= 5 and (o[raw == 100.0] == 1.0).all()
    assert (raw == -100.0).sum() >= 5 and (o[raw == -100.0] == 0.0).all()
    assert (o[raw == -5.6] < 1.0 / 255.0).all() and (o[raw == -5.5] > 1.0 / 255.0).all() and (o[raw == 4.6] > 0.99).all()
    assert (c.inp["scales"].numpy()[c.g.scaling.numpy() == -100.0] == 0.0).all()
    rot = c.inp["rotations"].numpy()
    assert (~rot.any(1)).sum() >= 5 and (np.abs(rot).sum(1) == np.float32(1e-8)).sum() >= 5
    # the oracle stays finite on all of it
    assert np.isfinite(c.run.color).all() and np.isfinite(c.run.language).all()
    gc, gl = grad_seed(c.st.image_height, c.st.image_width, seed=7)
    for k, v in c.run.backward(gc, gl if c.include_feature else None).items():
        assert np.isfinite(v).all(), k


def test_plain_scene_misses_the_edges():
    """What the census is for: the scenes of the rest of the suite do not pass it."""
    st, inp = scene(P=400, W=96, H=64, seed=0, sh_degree=3, scale_range=(0.03, 0.2))
    census = blend_census(st, inp, oracle.forward(st, **inp))
    assert census["blends"] > 10000 and census["saturated"] == 0 and census["o_zero"] == 0, census
    with pytest.raises(AssertionError):
        assert_reaches_edges(census)


def _dense(c, dt):
    st = c.st._replace(bg=c.st.bg.to(dt), viewmatrix=c.st.viewmatrix.to(dt), projmatrix=c.st.projmatrix.to(dt),
                       campos=c.st.campos.to(dt))
    leaves = {k: v.to(dt).clone().requires_grad_(True) for k, v in c.inp.items()}
    m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
    out = torch_ref.rasterize(st, leaves["means3D"], m2, leaves["opacities"], shs=leaves["shs"],
                              language_feature=leaves["language_feature_precomp"], scales=leaves["scales"],
                              rotations=leaves["rotations"])
    return leaves, m2, out


@pytest.mark.parametrize("name", sorted(EDGE_SCENES))
def test_forward_matches_dense_reference(name):
    c = edge_case(name)
    assert_reaches_edges(c.census, c.include_feature)
    with torch.no_grad():
        _, _, (color, lang, radii, ncon) = _dense(c, torch.float32)
    np.testing.assert_array_equal(radii.numpy(), c.run.radii)
    np.testing.assert_array_equal(ncon.numpy(), c.run.get("n_contrib"))
    print(name, "forward error", float(np.abs(color.numpy() - c.run.color).max()),
          float(np.abs(lang.numpy() - c.run.language).max()))
    np.testing.assert_allclose(color.numpy(), c.run.color, atol=2e-5, rtol=0)
    np.testing.assert_allclose(lang.numpy(), c.run.language, atol=2e-5, rtol=0)


@pytest.mark.parametrize("name", sorted(EDGE_SCENES))
def test_backward_matches_autograd_of_dense_reference(name):
    """Hand-derived oracle backward == torch.autograd through the dense formulation (float64), with
    the straight-through clamp, the division by 1 - alpha = 0.01, the clamped-colour mask and the
    degenerate rows all in the scene."""
    c = edge_case(name)
    assert_reaches_edges(c.census, c.include_feature)
    H, W = c.st.image_height, c.st.image_width
    gc, gl = grad_seed(H, W, seed=7)
    ograd = c.run.backward(gc, gl if c.include_feature else None)
    leaves, m2, (color, lang, radii, ncon) = _dense(c, torch.float64)
    np.testing.assert_array_equal(ncon.numpy(), c.run.get("n_contrib"))
    ((color * gc.double()).sum() + (lang * gl.double()).sum()).backward()
    checks = {k: leaves[k].grad for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    checks["means2D"] = m2.grad
    if c.include_feature:
        checks["language_feature_precomp"] = leaves["language_feature_precomp"].grad
    for k, ref in checks.items():
        ref = ref.numpy()
        assert np.max(np.abs(ref)) > 0, k
        err = np.max(np.abs(ograd[k] - ref)) / (np.max(np.abs(ref)) + 1e-12)
        print(name, k, "gradient error", err)
        assert err < 2e-4, (k, err)
