"""float64 CPU reference of SSIM (pytorch_msssim.ssim's definition), straight from the definition: the
forward slides the 2-D window outer(g, g) over the image with numpy (no convolution routine), the gradient is float64
torch autograd over an unfold-based restatement of the same definition.  The two forwards agree to about 1e-15."""
import numpy as np
import torch
from numpy.lib.stride_tricks import sliding_window_view

K1, K2 = 0.01, 0.03
C1, C2 = K1 * K1, K2 * K2   # data_range 1


def window(win_size=11, win_sigma=1.5):
    c = np.arange(win_size, dtype=np.float64) - win_size // 2
    g = np.exp(-(c * c) / (2.0 * win_sigma ** 2))
    return g / g.sum()


def ssim_nc(X, Y, win_size=11, win_sigma=1.5, c1=C1, c2=C2):
    """(N, C) float64 tensor: the mean SSIM map per image and channel of (N, C, H, W) tensors."""
    x, y = X.detach().double().cpu().numpy(), Y.detach().double().cpu().numpy()
    g2 = np.outer(window(win_size, win_sigma), window(win_size, win_sigma))

    def filt(a):
        return np.einsum("nchwij,ij->nchw", sliding_window_view(a, (win_size, win_size), axis=(2, 3)), g2)

    mu1, mu2 = filt(x), filt(y)
    s1, s2, s12 = filt(x * x) - mu1 * mu1, filt(y * y) - mu2 * mu2, filt(x * y) - mu1 * mu2
    smap = (2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * (2 * s12 + c2) / (s1 + s2 + c2)
    return torch.from_numpy(smap.reshape(*smap.shape[:2], -1).mean(-1))


def ssim_nc_unfold(X, Y, win_size=11, win_sigma=1.5, c1=C1, c2=C2):
    """The same definition as differentiable float64 torch ops: every window unfolded into a column."""
    x, y = X.double(), Y.double()
    N, C, H, W = x.shape
    g = torch.from_numpy(window(win_size, win_sigma))
    g2 = torch.outer(g, g).reshape(1, -1, 1)

    def filt(a):
        cols = torch.nn.functional.unfold(a.reshape(N * C, 1, H, W), win_size)   # (N*C, win^2, Np)
        return (cols * g2).sum(1).view(N, C, -1)

    mu1, mu2 = filt(x), filt(y)
    s1, s2, s12 = filt(x * x) - mu1 * mu1, filt(y * y) - mu2 * mu2, filt(x * y) - mu1 * mu2
    smap = (2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * (2 * s12 + c2) / (s1 + s2 + c2)
    return smap.mean(-1)


def grads(X, Y, win_size=11, win_sigma=1.5, c1=C1, c2=C2):
    """(d ssim[n, c] / d X, d ssim[n, c] / d Y), each (N, C, H, W) float64: a plane's pixels reach only its own value,
    so one backward of the sum gives every plane's gradient."""
    x = X.detach().double().cpu().requires_grad_(True)
    y = Y.detach().double().cpu().requires_grad_(True)
    ssim_nc_unfold(x, y, win_size, win_sigma, c1, c2).sum().backward()
    return x.grad, y.grad


def images(shape, seed, noise=0.1):
    """Uniform random X and Y = clamp(X + noise * randn), fp32 (N, C, H, W)."""
    gen = torch.Generator().manual_seed(seed)
    X = torch.rand(shape, generator=gen)
    Y = (X + noise * torch.randn(shape, generator=gen)).clamp(0, 1)
    return X, Y


def ssim_fp32_conv(X, Y, win_size=11, win_sigma=1.5, c1=C1, c2=C2):
    """What a user would otherwise run: pytorch_msssim's chain of five separable fp32 conv2d filters, (N, C) fp32."""
    x, y = X.float(), Y.float()
    C = x.shape[1]
    g = torch.from_numpy(window(win_size, win_sigma)).to(x)
    gh, gw = g.view(1, 1, -1, 1).repeat(C, 1, 1, 1), g.view(1, 1, 1, -1).repeat(C, 1, 1, 1)

    def filt(a):
        return torch.nn.functional.conv2d(torch.nn.functional.conv2d(a, gh, groups=C), gw, groups=C)

    mu1, mu2 = filt(x), filt(y)
    mu11, mu22, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = filt(x * x) - mu11, filt(y * y) - mu22, filt(x * y) - mu12
    cs = (2 * s12 + c2) / (s1 + s2 + c2)
    return (((2 * mu12 + c1) / (mu11 + mu22 + c1)) * cs).flatten(2).mean(-1)
