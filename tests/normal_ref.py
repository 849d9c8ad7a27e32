"""Reference of the density-gradient / normal-map tests: (sigma, d sigma / d x) of MetaNGP.density restated in torch
ops that autograd differentiates in the world points, in any float dtype.

sigma_grad(x, tensors, table, res, log2T, interp, amin, ext, dtype, weights):
  unit coordinates u = (x - amin) / ext, x01 = clamp(u, eps, 1 - eps), the hash grid of input_grad_ref.hashgrid,
  the two ReLU layers of the sigma trunk and the sigma head as ``dtype`` linears on the module's tensors, and
  TruncExp: sigma = exp(clamp(s, +-88.722839111)) with backward g * sigma also where s was clamped.
  weights="fp32":  u, x01 and the clamp's pass mask (eps <= u <= 1 - eps, torch's clamp backward) come from the
                   float32 arithmetic the kernel performs and are then promoted, x01 = x01_32 + pass * (x - x.detach())
                   / ext -- the same idea as the fp32 cells of input_grad_ref.  In float64 this is what the kernel is
                   compared with; in float32 (on the CPU) it is the restatement whose own error sets the tolerance.
  weights="exact": everything in ``dtype`` (for finite differences).
  Returns (sigma (M,), grad (M, 3), pre (M, 128)): pre holds every hidden pre-activation of both trunk layers, so a
  caller can set aside the samples that sit on a ReLU kink, where the gradient is discontinuous.

normal_composite(grad, weights, dtype): n = sum_s w_s * (-g_s / max(|g_s|, 1e-9)) with the terms in ``dtype`` and the
  sum over the samples in float64.
"""
import torch

import input_grad_ref as R

TRUNC = 88.722839111
KEYS = ("sigma_trunk.0.linear.weight", "sigma_trunk.0.linear.bias", "sigma_trunk.1.linear.weight",
        "sigma_trunk.1.linear.bias", "sigma_head.weight", "sigma_head.bias")


def sigma_grad(x, tensors, table, res, log2T, interp, amin, ext, eps=1e-6, dtype=torch.float64, weights="fp32"):
    dev = x.device
    w0, b0, w1, b1, wh, bh = [tensors[k].detach().to(dev, dtype) for k in KEYS]
    xr = x.detach().to(dtype).requires_grad_()
    mn = torch.as_tensor(amin, dtype=torch.float32, device=dev)
    ex = torch.as_tensor(ext, dtype=torch.float32, device=dev)
    lo = torch.tensor(eps, dtype=torch.float32, device=dev)
    hi = 1.0 - lo                                              # fp32, as MetaNGP._world_to_unit forms it
    if weights == "fp32":
        u32 = (x.detach().to(torch.float32) - mn) / ex
        x01_32 = u32.clamp(lo, hi)
        passed = ((u32 >= lo) & (u32 <= hi)).to(dtype)
        x01 = x01_32.to(dtype) + passed * (xr - xr.detach()) / ex.to(dtype)
    else:
        x01 = ((xr - mn.to(dtype)) / ex.to(dtype)).clamp(float(lo), float(hi))
    h0 = R.hashgrid(x01, table.detach().to(dev), res, log2T, interp, dtype=dtype, weights=weights)
    z1 = h0 @ w0.t() + b0
    z2 = torch.relu(z1) @ w1.t() + b1
    s = (torch.relu(z2) @ wh.t() + bh).squeeze(-1)
    sc = s + (s.clamp(-TRUNC, TRUNC) - s).detach()             # the clamped value with TruncExp's pass-through backward
    sigma = torch.exp(sc)
    (grad,) = torch.autograd.grad(sigma.sum(), xr)
    return sigma.detach(), grad, torch.cat([z1, z2], -1).detach()


def normal_composite(grad, weights, dtype=torch.float64):
    N, S = weights.shape
    g = grad.reshape(N, S, 3).to(dtype)
    d = g.norm(dim=-1, keepdim=True).clamp_min(1e-9)
    terms = weights.to(dtype).unsqueeze(-1) * (-g / d)
    return terms.double().sum(1)
