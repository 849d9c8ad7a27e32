"""Time the fused importance resampling (acn_resample_pdf through sample_pdf) against the torch-op
restatement of the same definition (ray_rendering._sample_pdf_torch: float64 cumsum, searchsorted, four gathers, cat
and sort, plus the torch expression of the sample points), in one process.

Sizes: 4096 rays at 64 coarse + 128 fine and at 256 + 128 samples.  Weights come from compositing a sparse density; t
is offset by 100; the fine quantiles are jittered.  One call returns (t_fine, t_merged, the (N * (S + F), 6) points).

Candidates alternated call by call (HIP events around every call, 5 warm-ups, median of 50, twice over -- the
difference of a candidate's two medians is the run-to-run spread the ratio is read against).  The torch chain is the
yardstick: the fused path stays sample_pdf's default only if its slower round is not slower than the torch chain's
faster round at either size.

For orientation only (no criterion): the eval render_rays of the C2 model (bench.py's single expert, 4096 rays) at
64 + 128 hierarchical against 256 stratified samples.

python tools/bench_resample.py [--out profiles/bench_resample.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from adaptive_city_nerf_amd import render_rays, sample_pdf  # noqa: E402
from adaptive_city_nerf_amd import ray_rendering as RR  # noqa: E402


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


def inputs(N, S, F, dev, gen):
    u = (torch.arange(S, device=dev).float()[None, :] + torch.rand(N, S, device=dev, generator=gen)) / S
    t = 100.0 + 2.0 + 30.0 * u
    d = torch.cat([t[:, 1:] - t[:, :-1], t[:, -1:] - t[:, -2:-1]], 1)
    sigma = torch.rand(N, S, device=dev, generator=gen) * 4.0 * (torch.rand(N, S, device=dev, generator=gen) < 0.3)
    alpha = 1.0 - torch.exp(-sigma * d)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha], -1), -1)[:, :-1]
    rays = torch.randn(N, 8, device=dev, generator=gen)
    rays[:, 6], rays[:, 7] = 102.0, 132.0
    return (alpha * T).float(), t, torch.rand(N, F, device=dev, generator=gen), rays


def torch_chain(t, w, F, jitter, rays):
    t_fine, t_merged = RR._sample_pdf_torch(t, w, F, jitter)
    return t_fine, t_merged, RR._points6(rays, t_merged)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "bench_resample.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample needs a HIP device"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "HIP events per call, candidates alternated, 5 warm-ups, median of 50, two rounds (ms)",
              "sizes": {}}
    worst = 0.0
    for N, S, F in ((4096, 64, 128), (4096, 256, 128)):
        w, t, jitter, rays = inputs(N, S, F, dev, gen)
        cands = {"fused": lambda: sample_pdf(t, w, F, jitter, rays=rays),
                 "torch": lambda: torch_chain(t, w, F, jitter, rays)}
        assert RR.FUSED_RESAMPLE
        gf, gt = cands["fused"](), cands["torch"]()
        dt = float((gf[0] - gt[0]).abs().max() / gt[0].abs().max())
        assert torch.equal(gf[1], torch.sort(torch.cat([t, gf[0]], 1), 1).values)
        assert torch.equal(gf[2], RR._points6(rays, gf[1]))
        med = alternate(cands)
        ratio = max(med["fused"]) / min(med["torch"])
        worst = max(worst, ratio)
        name = f"{N} rays, {S} + {F}"
        result["sizes"][name] = {"rays": N, "coarse": S, "fine": F, "ms": med,
                                 "fused_slower_round_over_torch_faster_round": ratio,
                                 "max_t_fine_difference_over_max_t": dt}
        print(f"{name:22s} fused {med['fused'][0]:.4f} / {med['fused'][1]:.4f} ms, torch {med['torch'][0]:.4f} / "
              f"{med['torch'][1]:.4f} ms, fused (slower round) / torch (faster round) = {ratio:.3f}; t_fine differs by "
              f"{dt:.1e} of the largest t")
    result["fused_kept_as_default"] = worst <= 1.0
    # orientation: the eval render of the C2 model, 64 + 128 hierarchical against 256 stratified samples
    import bench
    model, gbox, scene, sc = bench.build_model(dev, 1)
    model.eval()
    rays = bench.make_rays(scene, gbox, dev, 4096, 7)
    with torch.no_grad():
        cands = {"hierarchical 64 + 128": lambda: render_rays(model, rays, ray_samples=64, n_importance=128),
                 "stratified 256": lambda: render_rays(model, rays, ray_samples=256)}
        med = alternate(cands)
        a_h, a_s = cands["hierarchical 64 + 128"](), cands["stratified 256"]()
    result["render_c2_eval_4096_rays"] = {"ms": med, "note": "orientation only: different sample sets, not a criterion",
                                          "max_rgb_difference": float((a_h[0] - a_s[0]).abs().max())}
    print("C2 eval render, 4096 rays: " + ", ".join(f"{n} {v[0]:.3f} / {v[1]:.3f} ms" for n, v in med.items()))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
