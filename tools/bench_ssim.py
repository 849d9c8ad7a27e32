"""Time the fused SSIM (acn_ssim_fwd) against what a user would otherwise run, in one process.

Candidates, each one call of (N, C, H, W) fp32 images -> (N, C) values:
  fused            ops.ssim_fwd, value only (two launches)
  fused + grad     ops.ssim_fwd(want_grad=True): value and d ssim / d X (three launches)
  torch float64    metrics._ssim_torch: the same formula as float64 conv2d ops (CPU tensors, second_order())
  fp32 conv chain  pytorch_msssim's chain restated: five separable fp32 conv2d filters and the elementwise map

Sizes: 1 x 3 x 1080 x 1920 (one full-HD validation frame) and 8 x 3 x 128 x 128 (a batch of training patches).
Candidates alternated call by call (HIP events around every call, 5 warm-ups, median of 20, twice over -- the difference
of a candidate's two medians is the run-to-run spread a ratio is read against).  For orientation the distance of the fp32
chain and of the fused value from the float64 torch form is recorded too.

python tools/bench_ssim.py [--out profiles/bench_ssim.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from adaptive_city_nerf_amd import metrics, ops  # noqa: E402

C1, C2 = 0.01 ** 2, 0.03 ** 2


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(cands, warmup=5, iters=20, rounds=2):
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


def fp32_chain(x, y, gh, gw):
    C = x.shape[1]

    def filt(a):
        return F.conv2d(F.conv2d(a, gh, groups=C), gw, groups=C)

    mu1, mu2 = filt(x), filt(y)
    mu11, mu22, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = filt(x * x) - mu11, filt(y * y) - mu22, filt(x * y) - mu12
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return (((2 * mu12 + C1) / (mu11 + mu22 + C1)) * cs).flatten(2).mean(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "bench_ssim.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ssim needs a HIP device"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "HIP events per call, candidates alternated, 5 warm-ups, median of 20, two rounds (ms)",
              "sizes": {}}
    for shape in ((1, 3, 1080, 1920), (8, 3, 128, 128)):
        x = torch.rand(shape, device=dev, generator=gen)
        y = (x + 0.1 * torch.randn(shape, device=dev, generator=gen)).clamp(0, 1)
        g = metrics._gauss_window(11, 1.5, dev).float()
        gh, gw = g.view(1, 1, -1, 1).repeat(shape[1], 1, 1, 1), g.view(1, 1, 1, -1).repeat(shape[1], 1, 1, 1)
        cands = {"fused": lambda: ops.ssim_fwd(x, y, c1=C1, c2=C2)[0],
                 "fused + grad": lambda: ops.ssim_fwd(x, y, c1=C1, c2=C2, want_grad=True)[0],
                 "torch float64": lambda: metrics._ssim_torch(x, y, 11, 1.5, C1, C2),
                 "fp32 conv chain": lambda: fp32_chain(x, y, gh, gw)}
        ref = metrics._ssim_torch(x.double(), y.double(), 11, 1.5, C1, C2)
        dist = {n: float(((cands[n]().double() - ref).abs() / ref.abs()).max() / 2.0 ** -24)
                for n in ("fused", "fp32 conv chain")}
        med = alternate(cands)
        ratio = max(med["fused"]) / min(med["fp32 conv chain"])
        name = "x".join(str(s) for s in shape)
        result["sizes"][name] = dict(ms=med, fused_slower_round_over_fp32_chain_faster_round=ratio,
                                     distance_from_float64_in_units_of_2pow_minus24_relative=dist,
                                     workspace_bytes={"value": int(ops._lib.lib().acn_ssim_workspace_bytes(*shape, 0)),
                                                      "with gradient": int(ops._lib.lib().acn_ssim_workspace_bytes(*shape, 1))})
        print(f"{name}: " + ", ".join(f"{n} {v[0]:.4f} / {v[1]:.4f} ms" for n, v in med.items()))
        print(f"{name}: fused (slower round) / fp32 chain (faster round) = {ratio:.3f}; distance from float64 in 2^-24 "
              f"relative: fused {dist['fused']:.2f}, fp32 chain {dist['fp32 conv chain']:.2f}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
