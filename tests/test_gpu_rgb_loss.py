"""The RGB stage's fused loss (langsplat_amd.rgb_loss / ssim: lsr_rgb_loss_forward / _backward)
against the fp64 restatement of tests/rgb_loss_ref.py.

Yardstick (DESIGN §6a/§6b's rule): e_ref is the fp32 restatement against the fp64 one on the case's
own input, taken separately for the SSIM map and for the gradient (compared as N * dL/dimage); the
bound is 8 e_ref.  Planes under 256 pixels take the e_ref of the (3, TH+1, TW+1) case of their kind;
the *equal* kind (gt = image.clone(): its own map e_ref is exactly 0) takes the *rand* e_ref of its
shape.  The three scalars: rtol 1e-5 against fp64."""
import numpy as np
import pytest
import torch

import bench
from langsplat_amd import _native, loss as L, rgb_loss, ssim
from langsplat_amd.synthetic import make_cameras, make_gaussians
from tests import rgb_loss_ref as R
from tests.test_gpu_parity import assert_grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
TH, TW = _native.RGB_LOSS_TILE
SHAPES = [(1, 1, 1), (3, 3, 7), (3, 5, 5), (1, 11, 11), (3, TH, TW), (3, TH + 1, TW + 1), (3, 2 * TH + 1, TW - 1),
          (2, 40, 130), (3, 96, 128), (2, 3, 17, 65)]
LAMBDA = 0.2


def bounds(kind, shape):
    """(map bound, gradient bound) = 8 e_ref of the case the yardstick names for (kind, shape)."""
    ref_kind = "rand" if kind == "equal" else kind
    ref_shape = (3, TH + 1, TW + 1) if shape[-2] * shape[-1] < 256 else shape
    r = R.reference(ref_kind, ref_shape, LAMBDA)
    return 8.0 * r["e_map"], 8.0 * r["e_grad"]


def run_gpu(image, gt, scale=1.0):
    """loss terms, SSIM map and N * dL/dimage of the fused path, all on the CPU in fp64."""
    x = image.detach().to(DEV).requires_grad_(True)
    y = gt.to(DEV)
    loss, l1, s = rgb_loss(x, y, LAMBDA, return_terms=True)
    (scale * loss).backward()
    planes, H, W = x.numel() // (x.shape[-1] * x.shape[-2]), x.shape[-2], x.shape[-1]
    _, _, smap = L._rgb_forward(x.detach(), y, planes, H, W, LAMBDA, False, want_ssim_map=True)
    return {"loss": loss.detach().double().cpu(), "l1": l1.double().cpu(), "ssim": s.double().cpu(),
            "map": smap.double().cpu().reshape(image.shape), "ngrad": x.grad.double().cpu() * x.numel() / scale}


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", R.KINDS)
def test_parity_with_fp64(kind, shape):
    ref = R.reference(kind, shape, LAMBDA)
    got = run_gpu(ref["image"], ref["gt"])
    b_map, b_grad = bounds(kind, shape)
    e_map = float((got["map"] - ref["f64"]["map"]).abs().max())
    e_grad = float((got["ngrad"] - ref["f64"]["ngrad"]).abs().max())
    rel = {k: abs(float(got[k]) - float(ref["f64"][k])) / max(abs(float(ref["f64"][k])), 1e-300)
           for k in ("loss", "l1", "ssim")}
    print(f"rgb_loss {kind} {shape}: map err {e_map:.3g} (e_ref {b_map / 8:.3g}) grad err {e_grad:.3g} "
          f"(e_ref {b_grad / 8:.3g}) max|N grad| {float(ref['f64']['ngrad'].abs().max()):.3g} "
          f"rel loss {rel['loss']:.2g} l1 {rel['l1']:.2g} ssim {rel['ssim']:.2g}")
    assert e_map <= b_map
    assert e_grad <= b_grad
    for k in ("loss", "l1", "ssim"):
        torch.testing.assert_close(got[k], ref["f64"][k], rtol=1e-5, atol=0, msg=lambda m, k=k: f"{k}: {m}")
    # ssim() is the same forward with lambda = 1
    s = ssim(ref["image"].to(DEV), ref["gt"].to(DEV))
    assert float(s) == float(got["ssim"])
    if kind == "equal":
        assert float(got["l1"]) == 0.0
        assert bool(torch.isfinite(got["ngrad"]).all())


@pytest.mark.parametrize("kind", ["rand", "smooth"])
def test_scaled_loss_and_upstream_op_stay_within_the_bound(kind):
    shape = (3, TH + 1, TW + 1)
    ref = R.reference(kind, shape, LAMBDA)
    _, b_grad = bounds(kind, shape)
    got = run_gpu(ref["image"], ref["gt"], scale=3.0)
    assert float((got["ngrad"] - ref["f64"]["ngrad"]).abs().max()) <= b_grad
    # image = 0.5 * raw (exact in fp32): d/draw = 0.5 d/dimage
    raw = (2.0 * ref["image"]).to(DEV).requires_grad_(True)
    rgb_loss(0.5 * raw, ref["gt"].to(DEV), LAMBDA).backward()
    ngrad = 2.0 * raw.grad.double().cpu() * raw.numel()
    assert float((ngrad - ref["f64"]["ngrad"]).abs().max()) <= b_grad


def _everything(x, y):
    """terms, maps and gradient of one forward + backward, as device tensors."""
    x = x.detach().clone().requires_grad_(True)
    loss, l1, s = rgb_loss(x, y, LAMBDA, return_terms=True)
    maps = loss.grad_fn.saved_tensors[2]
    loss.backward()
    return torch.stack([loss.detach(), l1, s]), maps, x.grad


def test_calls_are_bit_identical_also_on_a_side_stream():
    ref = R.reference("rand", (3, 96, 128), LAMBDA)
    x, y = ref["image"].to(DEV), ref["gt"].to(DEV)
    a, b = _everything(x, y), _everything(x, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _everything(x, y)
    side.synchronize()
    torch.cuda.synchronize()
    for other in (b, c):
        for u, v in zip(a, other):
            assert torch.equal(u, v)


def test_no_gradient_path_returns_the_same_terms():
    ref = R.reference("smooth", (3, 2 * TH + 1, TW - 1), LAMBDA)
    x, y = ref["image"].to(DEV), ref["gt"].to(DEV)
    want = torch.stack(rgb_loss(x.clone().requires_grad_(True), y, LAMBDA, return_terms=True)).detach()
    plain = rgb_loss(x, y, LAMBDA, return_terms=True)
    assert not plain[0].requires_grad
    with torch.no_grad():
        quiet = rgb_loss(x.clone().requires_grad_(True), y, LAMBDA, return_terms=True)
    assert not quiet[0].requires_grad
    assert torch.equal(torch.stack(plain), want) and torch.equal(torch.stack(quiet), want)
    # lambda = 1: the loss is 1 - ssim
    s = ssim(x, y)
    assert float(s) == float(want[2])


def test_graph_capture_replays_the_eager_result():
    shape = (3, TH + 1, TW + 1)
    first, second = R.reference("rand", shape, LAMBDA), R.reference("smooth", shape, LAMBDA)
    y = torch.empty(shape, device=DEV)
    x = torch.empty(shape, device=DEV, requires_grad=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        x.copy_(first["image"])
        y.copy_(first["gt"])
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up on the capture stream: the scratch of that stream exists before capture
            x.grad = None
            rgb_loss(x, y, LAMBDA).backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(g, stream=s):
        loss, l1, sv = rgb_loss(x, y, LAMBDA, return_terms=True)
        loss.backward()
    static = (loss.detach(), l1, sv, x.grad)
    with torch.no_grad():
        x.copy_(second["image"])
        y.copy_(second["gt"])
    g.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in static]
    terms, _, grad = _everything(second["image"].to(DEV), second["gt"].to(DEV))
    assert torch.equal(torch.stack(replayed[:3]), terms)
    assert torch.equal(replayed[3], grad)


def test_error_cases():
    a = torch.zeros((3, 8, 8), device=DEV)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rgb_loss(a.cpu(), a.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        rgb_loss(a, a.cpu())
    with pytest.raises(ValueError, match=r"\(C,H,W\) or \(B,C,H,W\)"):
        rgb_loss(a, torch.zeros((3, 8, 9), device=DEV))
    with pytest.raises(ValueError, match=r"\(C,H,W\) or \(B,C,H,W\)"):
        rgb_loss(a[0], a[0])
    with pytest.raises(ValueError, match=r"\(C,H,W\) or \(B,C,H,W\)"):
        ssim(a[None, None], a[None, None])
    with pytest.raises(ValueError, match="gt requires grad"):
        rgb_loss(a, a.clone().requires_grad_(True))


class FusedRGBStep(bench.RGBStep):
    """bench.RGBStep with the loss of train.py:100-103 as rgb_loss."""

    def __call__(self):
        pkg = bench.render(self.cam, self.model, bench.Pipe, self.bg, bench.OptRGB)
        loss = rgb_loss(pkg["render"], self.gt, bench.OptRGB.lambda_dssim)
        loss.backward()
        _native.densification_stats(pkg["radii"], pkg["viewspace_points"].grad, self.max_radii2D,
                                    self.xyz_gradient_accum, self.denom)
        self.optim.step()
        self.optim.zero_grad(set_to_none=True)
        return loss


def test_rgb_step_with_the_fused_loss_matches_bench_rgb_step():
    """The scene of test_gpu_rgb_step.py: loss within rtol 1e-5, the six gradients as Adam receives
    them within the parity tolerance, the densification statistics equal (radii and counts exactly;
    the accumulated gradient norms, which are sums of those gradients, within their tolerance)."""
    W, H, P = 128, 96, 3000
    cam = make_cameras(1, W, H, device=DEV)[0]
    gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(5)).to(DEV)
    out = {}
    for name, cls in (("torch", bench.RGBStep), ("fused", FusedRGBStep)):
        step = cls(make_gaussians(P, seed=16, scale_range=(0.02, 0.12)).to(DEV), cam, gt)
        grads = {}
        orig = step.optim.step

        def spy(*a, _step=step, _grads=grads, _orig=orig, **kw):
            for grp in _step.optim.param_groups:
                _grads[grp["name"]] = grp["params"][0].grad.detach().clone()
            return _orig(*a, **kw)
        step.optim.step = spy
        loss = step()
        torch.cuda.synchronize()
        out[name] = (loss.detach(), grads, step)
    torch.testing.assert_close(out["fused"][0], out["torch"][0], rtol=1e-5, atol=0)
    assert sorted(out["fused"][1]) == ["f_dc", "f_rest", "opacity", "rotation", "scaling", "xyz"]
    for k, g in out["fused"][1].items():
        assert_grad_close(k, g.cpu().numpy(), out["torch"][1][k].cpu().numpy())
    fs, ts = out["fused"][2], out["torch"][2]
    torch.testing.assert_close(fs.max_radii2D, ts.max_radii2D, rtol=0, atol=0)
    torch.testing.assert_close(fs.denom, ts.denom, rtol=0, atol=0)
    assert float(ts.denom.sum()) > 0
    assert_grad_close("xyz_gradient_accum", fs.xyz_gradient_accum.cpu().numpy(), ts.xyz_gradient_accum.cpu().numpy())
    assert np.isfinite(float(out["fused"][0]))
