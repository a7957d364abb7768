"""CPU references for the RGB stage's loss kernels (lsr_rgb_loss_forward / _backward, include/lsr.h):
train.py:100-103 with utils/loss_utils.py:17-18 and :23-63 (size_average=True), restated in torch
at a chosen precision.

  taps               the 11 Gaussian taps (sigma 1.5): normalised in fp64 and rounded to fp32, the
                     values bench.ssim and the kernels use (the reference normalises in fp32, which
                     moves the two taps next to the centre by one ulp)
  loss_terms         the reference's op sequence: one 11 x 11 depthwise conv2d with padding=5 per
                     windowed mean, the window g g^T formed at the working precision; returns loss,
                     l1, ssim and the SSIM map
  closed_form_grad   dL/dimage from the three partial-derivative maps the kernels use
  make_case          the seeded inputs of the tests: kinds rand / smooth / const / equal
  reference          per case, cached: fp64 and fp32 results and their difference e_ref
"""
from functools import lru_cache

import torch

F = torch.nn.functional
WINDOW, PAD, SIGMA = 11, 5, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
KINDS = ("rand", "smooth", "const", "equal")


def taps(dtype=torch.float64):
    d = torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2
    g = torch.exp(-d * d / (2 * SIGMA ** 2))
    return (g / g.sum()).float().to(dtype)


def _planes(t):
    """(C,H,W) or (B,C,H,W) -> (1, planes, H, W): every plane is filtered on its own."""
    return t.reshape(1, -1, t.shape[-2], t.shape[-1])


def windowed_mean(t, window):
    """The 11 x 11 zero-padded window over each plane of t (1, planes, H, W)."""
    n = t.shape[1]
    return F.conv2d(t, window.expand(n, 1, WINDOW, WINDOW).contiguous(), padding=PAD, groups=n)


def loss_terms(image, gt, lambda_dssim=0.2):
    """(loss, l1, ssim, ssim_map) at the precision of `image`; the map has image's shape."""
    x, y = _planes(image), _planes(gt)
    g = taps(image.dtype).view(WINDOW, 1)
    window = g.mm(g.t()).view(1, 1, WINDOW, WINDOW)
    mu1, mu2 = windowed_mean(x, window), windowed_mean(y, window)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = windowed_mean(x * x, window) - mu1_sq
    sigma2_sq = windowed_mean(y * y, window) - mu2_sq
    sigma12 = windowed_mean(x * y, window) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    ssim = ssim_map.mean()
    l1 = torch.abs(image - gt).mean()
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim)
    return loss, l1, ssim, ssim_map.reshape(image.shape)


def closed_form_grad(image, gt, lambda_dssim=0.2):
    """dL/dimage without autograd.  With A = 2 mu1 mu2 + C1, B = 2 s12 + C2, D = mu1^2 + mu2^2 + C1,
    E = s1 + s2 + C2, S = A B / (D E), and e11 = E[x^2], e12 = E[xy] as variables beside mu1:
        Ma = dS/dmu1 = 2 mu2 B / (D E) - 2 mu2 A / (D E) - 2 mu1 S / D + 2 mu1 S / E
        Mb = dS/de11 = -S / E
        Mc = dS/de12 = 2 A / (D E)
        dL/dx = (1 - l) / N sign(x - y) - l / N (conv(Ma) + 2 x conv(Mb) + y conv(Mc))."""
    x, y = _planes(image), _planes(gt)
    g = taps(image.dtype).view(WINDOW, 1)
    window = g.mm(g.t()).view(1, 1, WINDOW, WINDOW)
    mu1, mu2 = windowed_mean(x, window), windowed_mean(y, window)
    e11, e22, e12 = windowed_mean(x * x, window), windowed_mean(y * y, window), windowed_mean(x * y, window)
    A = 2 * mu1 * mu2 + C1
    B = 2 * (e12 - mu1 * mu2) + C2
    D = mu1 * mu1 + mu2 * mu2 + C1
    E = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2
    S = A * B / (D * E)
    Ma = 2 * mu2 * B / (D * E) - 2 * mu2 * A / (D * E) - 2 * mu1 * S / D + 2 * mu1 * S / E
    Mb = -S / E
    Mc = 2 * A / (D * E)
    N = x.numel()
    ds = windowed_mean(Ma, window) + 2 * x * windowed_mean(Mb, window) + y * windowed_mean(Mc, window)
    grad = (1.0 - lambda_dssim) / N * torch.sign(x - y) - lambda_dssim / N * ds
    return grad.reshape(image.shape)


def make_case(kind, shape, seed=0):
    """(image, gt) fp32 in [0, 1] of `shape` ((C,H,W) or (B,C,H,W))."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * len(shape) + sum(shape))
    if kind == "rand":
        return torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    if kind == "smooth":
        # a 5 x 5 box blur (clipped at the border) and the same image with noise of sigma 0.05: the
        # variances nearly cancel, as when a rendered image meets its photograph
        raw = torch.rand(shape, generator=gen)
        img = F.avg_pool2d(_planes(raw), 5, stride=1, padding=2, count_include_pad=False).reshape(shape)
        noisy = (img + 0.05 * torch.randn(shape, generator=gen)).clamp(0.0, 1.0)
        return img.contiguous(), noisy
    if kind == "const":
        return torch.full(shape, 0.5), torch.full(shape, 0.25)
    if kind == "equal":
        img = torch.rand(shape, generator=gen)
        return img, img.clone()
    raise ValueError(kind)


def _run(image, gt, lambda_dssim, dtype):
    x = image.detach().to(dtype).clone().requires_grad_(True)
    loss, l1, ssim, smap = loss_terms(x, gt.to(dtype), lambda_dssim)
    (grad,) = torch.autograd.grad(loss, x)
    return {"loss": loss.detach(), "l1": l1.detach(), "ssim": ssim.detach(), "map": smap.detach(),
            "ngrad": grad * x.numel()}


@lru_cache(maxsize=None)
def reference(kind, shape, lambda_dssim=0.2):
    """The case's inputs, its fp64 and fp32 results (gradient as N * dL/dimage, so every case is on
    one scale) and e_ref = max |fp32 - fp64| for the SSIM map and for the gradient.  Cached: treat
    as read-only."""
    image, gt = make_case(kind, shape)
    r64, r32 = _run(image, gt, lambda_dssim, torch.float64), _run(image, gt, lambda_dssim, torch.float32)
    return {"image": image, "gt": gt, "f64": r64, "f32": r32,
            "e_map": float((r32["map"].double() - r64["map"]).abs().max()),
            "e_grad": float((r32["ngrad"].double() - r64["ngrad"]).abs().max())}
