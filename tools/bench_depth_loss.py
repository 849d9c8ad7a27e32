"""Time the fused depth supervision (acn_depth_loss_dense / acn_depth_loss_packed) against the torch-op
restatement of the same formula (nerfacc._depth_loss_torch: float64 ops with torch.special.erf, what second_order() and
CPU tensors take), forward plus backward, in one process.

Sizes: 1000 x 96 (C5, one adaptation batch), 4096 x 256 (C2) and a packed batch of 4096 rays with ragged counts
(0 .. 255 samples, mean 128).  Weights come from compositing a sparse density; t is offset by 100; every ray has a
target inside its span and a half-width of 1.5 sample spacings.  One call is loss = f(weights); loss.sum().backward()
on weights that require grad.

Candidates alternated call by call (HIP events around every call, 5 warm-ups, median of 50, twice over -- the
difference of a candidate's two medians is the run-to-run spread the ratio is read against).  The torch chain is the
yardstick: the fused path is kept only where it is not slower.

python tools/bench_depth_loss.py [--out profiles/bench_depth_loss.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from adaptive_city_nerf_amd import depth_loss, nerfacc  # noqa: E402
from adaptive_city_nerf_amd.ray_rendering import second_order  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(cands, warmup=5, iters=50, rounds=2):
    """{name: [median of round 0, median of round 1, ...]} with the candidates alternated call by call."""
    out = {n: [] for n in cands}
    for _ in range(rounds):
        for _ in range(warmup):
            for fn in cands.values():
                fn()
        torch.cuda.synchronize()
        ts = {n: [] for n in cands}
        for _ in range(iters):
            for n, fn in cands.items():
                ts[n].append(timed(fn))
        for n in cands:
            out[n].append(statistics.median(ts[n]))
    return out


def composite(sigma, dt):
    alpha = 1.0 - torch.exp(-sigma * dt)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1.0 - alpha], -1), -1)[..., :-1]
    return (alpha * T).float()


def dense_inputs(N, S, dev, gen):
    u = (torch.arange(S, device=dev).float()[None, :] + torch.rand(N, S, device=dev, generator=gen)) / S
    t = 100.0 + 2.0 + 30.0 * u
    d = torch.cat([t[:, 1:] - t[:, :-1], t[:, -1:] - t[:, -2:-1]], 1)
    sigma = torch.rand(N, S, device=dev, generator=gen) * 4.0 * (torch.rand(N, S, device=dev, generator=gen) < 0.3)
    rays = torch.zeros(N, 8, device=dev)
    rays[:, 6], rays[:, 7] = 102.0, 132.0
    z = 102.0 + 30.0 * (0.25 + 0.5 * torch.rand(N, device=dev, generator=gen))
    eps = torch.full((N,), 1.5 * 30.0 / S, device=dev)
    return composite(sigma, d).requires_grad_(True), t, rays, z, eps


def packed_inputs(N, dev, gen):
    counts = torch.randint(0, 256, (N,), device=dev, generator=gen)
    ri = torch.repeat_interleave(torch.arange(N, device=dev), counts)
    M = int(ri.numel())
    dt = torch.rand(M, device=dev, generator=gen) * 0.2 + 1e-3
    first = (torch.cumsum(counts, 0) - counts).index_select(0, ri)
    end = torch.cumsum(dt.double(), 0)
    t1 = (end - (end - dt.double()).index_select(0, first) + 100.0).float()   # restarts at 100 on every ray
    t0 = t1 - dt
    sigma = torch.rand(M, device=dev, generator=gen) * 4.0 * (torch.rand(M, device=dev, generator=gen) < 0.3)
    w, _, _ = nerfacc.render_weight_from_density(t0, t1, sigma, ray_indices=ri, n_rays=N)
    z = 100.0 + 0.1 * counts.float() * (0.25 + 0.5 * torch.rand(N, device=dev, generator=gen)) + 0.01
    eps = torch.full((N,), 0.15, device=dev)
    return w.detach().requires_grad_(True), t0, t1, ri, M, z, eps


def step(fn, w, torch_form):
    def run():
        w.grad = None
        with second_order(torch_form):
            fn().sum().backward()
        return w.grad
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "bench_depth_loss.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_loss needs a HIP device"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "HIP events per forward + backward call, candidates alternated, 5 warm-ups, median of 50, two "
                        "rounds (ms)", "sizes": {}}
    cases = {}
    for name, (N, S) in (("dense 1000x96 (C5)", (1000, 96)), ("dense 4096x256 (C2)", (4096, 256))):
        w, t, rays, z, eps = dense_inputs(N, S, dev, gen)
        f = lambda w=w, t=t, rays=rays, z=z, eps=eps: depth_loss(w, t, z, eps, rays=rays, reduction="none")   # noqa: E731
        cases[name] = (w, f, {"rays": N, "samples": N * S})
    N = 4096
    w, t0, t1, ri, M, z, eps = packed_inputs(N, dev, gen)
    f = lambda: nerfacc.depth_loss(w, t0, t1, z, eps, ray_indices=ri, n_rays=N)   # noqa: E731
    cases["packed 4096 rays, ragged"] = (w, f, {"rays": N, "samples": M})
    for name, (w, f, meta) in cases.items():
        cands = {"fused": step(f, w, False), "torch": step(f, w, True)}
        gf, gt = cands["fused"]().clone(), cands["torch"]().clone()
        dev_rel = float((gf - gt).abs().max() / gt.abs().max().clamp_min(1e-30))
        med = alternate(cands)
        ratio = max(med["fused"]) / min(med["torch"])
        result["sizes"][name] = dict(meta, ms=med, fused_slower_round_over_torch_faster_round=ratio,
                                     max_grad_difference_over_max_grad=dev_rel)
        print(f"{name:28s} fused {med['fused'][0]:.4f} / {med['fused'][1]:.4f} ms, torch {med['torch'][0]:.4f} / "
              f"{med['torch'][1]:.4f} ms, fused (slower round) / torch (faster round) = {ratio:.3f}; gradients differ by "
              f"{dev_rel:.1e} of their largest")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
