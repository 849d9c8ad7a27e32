"""Time the fused per-image affine colour loss (acn_appearance_mse through train.appearance_mse_loss)
against the composed torch chain on the same inputs (the correction as torch ops, then the colour transform and
F.mse_loss: what second_order() and CPU tensors take), forward plus backward to the prediction, the matrices and the
offsets, in one process.

Sizes: 4096 rays over 256 images (one adaptation batch) and 65536 rays over 2048 images (the large end of the design
point: every slot workgroup scans the whole slot column).  Predictions in [-0.2, 1.2], matrices near the identity,
uniform image indices with a tenth of the rays outside the table.  One call is loss = f(pred, A, b); loss.backward().
Also timed: the bare ops.appearance_mse launch (loss plus all gradients, no autograd around it) and the same launch
without gradients (the ray workgroups alone), whose difference is what the slot workgroups cost.

Candidates alternated call by call (HIP events around every call, 5 warm-ups, median of 50, twice over -- the
difference of a candidate's two medians is the run-to-run spread the ratio is read against).

python tools/bench_appearance.py [--out profiles/bench_appearance.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from adaptive_city_nerf_amd import AppearanceAffine, ops  # noqa: E402
from adaptive_city_nerf_amd.ray_rendering import second_order  # noqa: E402
from adaptive_city_nerf_amd.train import appearance_mse_loss  # noqa: E402


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


def inputs(N, I, dev, gen):
    pred = (torch.rand(N, 3, device=dev, generator=gen) * 1.4 - 0.2).requires_grad_(True)
    gt = torch.rand(N, 3, device=dev, generator=gen)
    app = AppearanceAffine(I, device=dev)
    with torch.no_grad():
        app.matrix.add_(0.15 * torch.randn(I, 3, 3, device=dev, generator=gen))
        app.offset.add_(0.05 * torch.randn(I, 3, device=dev, generator=gen))
    img = torch.randint(0, I + I // 9 + 1, (N,), device=dev, generator=gen).int()   # a tenth outside the table
    return pred, gt, app, img


def step(pred, gt, app, img, torch_form):
    def run():
        pred.grad = app.matrix.grad = app.offset.grad = None
        with second_order(torch_form):
            appearance_mse_loss(pred, gt, img, app, "linear").backward()
        return pred.grad, app.matrix.grad, app.offset.grad
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "bench_appearance.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_appearance needs a HIP device"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "HIP events per call, candidates alternated, 5 warm-ups, median of 50, two rounds (ms)",
              "sizes": {}}
    for N, I in ((4096, 256), (65536, 2048)):
        pred, gt, app, img = inputs(N, I, dev, gen)
        slots = app.slots(img)
        A, b, p = app.matrix.detach(), app.offset.detach(), pred.detach()
        cands = {"fused": step(pred, gt, app, img, False), "torch": step(pred, gt, app, img, True),
                 "launch": lambda: ops.appearance_mse(p, gt, slots, A, b),
                 "launch_no_grad": lambda: ops.appearance_mse(p, gt, slots, A, b, want_grad=False)}
        gf = [g.clone() for g in cands["fused"]()]
        gt_ = [g.clone() for g in cands["torch"]()]
        dev_rel = [float((u - v).abs().max() / v.abs().max().clamp_min(1e-30)) for u, v in zip(gf, gt_)]
        med = alternate(cands)
        ratio = max(med["fused"]) / min(med["torch"])
        result["sizes"][f"N {N}, I {I}"] = dict(
            rays=N, images=I, ms=med, fused_slower_round_over_torch_faster_round=ratio,
            max_grad_difference_over_max_grad=dict(zip(("pred", "matrix", "offset"), dev_rel)))
        print(f"N {N:6d}, I {I:5d}: fused {med['fused'][0]:.4f} / {med['fused'][1]:.4f} ms, torch "
              f"{med['torch'][0]:.4f} / {med['torch'][1]:.4f} ms, fused (slower round) / torch (faster round) = "
              f"{ratio:.3f}; the launch alone {med['launch'][0]:.4f} / {med['launch'][1]:.4f} ms, without gradients "
              f"{med['launch_no_grad'][0]:.4f} / {med['launch_no_grad'][1]:.4f} ms; gradients differ by "
              f"{max(dev_rel):.1e} of their largest")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
