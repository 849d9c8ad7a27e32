"""Time the eval renders from fp16 hash tables against the fp32 tables of the same build, in one process
(DESIGN.md §4q): set_render_table_dtype(torch.float16) against torch.float32 on the same model and rays.

Cases: the C2 batch (one expert, 4096 rays x 256 samples, log2T = 20), the C3 batch (4 experts, soft routing, the same
ray count and samples through the expert-sorted plan bench.py uses) and one C4-like frame (8 experts, --frame^2 rays x
96 samples, one GPU).  HIP events around every call, median of 20 after 5 warm-ups, the two modes alternating.  Per
case also max |rgb16 - rgb32| and the PSNR of the fp16 image against the fp32 image, on the bench table (formula
table, amplitude 0.5) and on the same table scaled to the default-init amplitude 1e-3 (where ~6 % of the entries are
fp16 subnormals).  The yardstick is the fp32 mode of this run, never a stored figure.  Prints a table and writes
profiles/bench_f16_table.json (or --out).

python tools/bench_f16_table.py [--rays N] [--samples S] [--frame F] [--cases c2,c3,c4] [--out PATH]
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import bench  # noqa: E402
from adaptive_city_nerf_amd import parallel, render_rays  # noqa: E402


def alternate_ms(fns, warmup=5, iters=20):
    """Median milliseconds of each callable, the callables taking turns (same machine state for all)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return [statistics.median(t) for t in ts]


def quality(rgb16, rgb32):
    d = (rgb16.double() - rgb32.double())
    mse = float((d * d).mean())
    return {"max_abs_rgb_diff": float(d.abs().max()), "psnr_db": None if mse == 0.0 else -10.0 * math.log10(mse)}


def run_case(name, model, render, samples):
    """render(): one call returning the rgb image / batch under the model's current mode."""
    def mode(dtype):
        def fn():
            for sub in model.submodules:   # the flag alone: set_render_table_dtype(float32) would free the fp16 copy
                sub.xyz_encoder._render_table_dtype = dtype   # and the next fp16 call convert the table again
            with torch.no_grad():
                return render()
        return fn

    model.set_render_table_dtype(torch.float16)

    f32, f16 = mode(torch.float32), mode(torch.float16)
    t32, t16 = alternate_ms([f32, f16])
    res = {"case": name, "ray_samples_per_call": samples, "fp32_ms": t32, "fp16_ms": t16, "fp16_over_fp32": t16 / t32,
           "fp32_ray_samples_per_s": samples / (t32 * 1e-3), "fp16_ray_samples_per_s": samples / (t16 * 1e-3),
           "bench_table_scale_0.5": quality(f16(), f32())}
    with torch.no_grad():     # the same tables at the default-init amplitude (hash_init_scale 1e-3), then restored
        saved = [sub.xyz_encoder.hash_table.detach().clone() for sub in model.submodules]
        for sub in model.submodules:
            sub.xyz_encoder.hash_table.mul_(1e-3 / 0.5)
        res["default_init_scale_1e-3"] = quality(f16(), f32())
        for sub, t in zip(model.submodules, saved):
            sub.xyz_encoder.hash_table.copy_(t)
    model.set_render_table_dtype(torch.float32)
    q = res["bench_table_scale_0.5"]
    print(f"{name}: fp32 {t32:.3f} ms, fp16 {t16:.3f} ms, fp16/fp32 {t16 / t32:.3f}; max|drgb| {q['max_abs_rgb_diff']:.2e}"
          f", PSNR {q['psnr_db'] if q['psnr_db'] is None else round(q['psnr_db'], 1)} dB (scale 0.5); "
          f"{res['default_init_scale_1e-3']} (scale 1e-3)", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--frame", type=int, default=800)
    ap.add_argument("--cases", default="c2,c3,c4")
    ap.add_argument("--out", default=str(REPO / "profiles" / "bench_f16_table.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_f16_table.py measures on a HIP device"
    dev = torch.device("cuda", 0)
    cases = a.cases.split(",")
    res = {"device": torch.cuda.get_device_name(0), "method": "HIP events per call, median of 20 after 5 warm-ups, "
           "fp32 and fp16 render tables alternating on the same model and rays", "cases": []}
    if "c2" in cases:
        model, gbox, scene, _ = bench.build_model(dev, 1)
        rays = bench.make_rays(scene, gbox, dev, a.rays, 1234)
        res["cases"].append(run_case(
            f"C2 (1 expert, {a.rays} x {a.samples})", model,
            lambda: render_rays(model, rays, ray_samples=a.samples, bg_color_default="white")[0], a.rays * a.samples))
        del model
    if "c3" in cases:
        model, gbox, scene, _ = bench.build_model(dev, 4)
        grays = bench.make_rays(scene, gbox, dev, a.rays, 1234)
        plan = parallel.expert_sorted_plan(parallel.expert_spatial_keys(grays, model), 1)

        def render_fn(r):
            rgb, depth, _, acc = render_rays(model, r, ray_samples=a.samples, bg_color_default="white",
                                             _want_weights=False)
            return rgb, depth, acc

        res["cases"].append(run_case(
            f"C3 (4 experts, {a.rays} x {a.samples})", model,
            lambda: parallel.render_rays_sharded(grays, render_fn, plan)[0], a.rays * a.samples))
        del model
    if "c4" in cases:
        model, gbox, scene, _ = bench.build_model(dev, 8)
        H, W, intr, c2w = bench.frame_camera(scene, a.frame, a.frame)
        res["cases"].append(run_case(
            f"C4-like (8 experts, {H}x{W} frame x 96)", model,
            lambda: parallel.render_image_sharded(model, H=H, W=W, fx=intr[0], fy=intr[1], cx=intr[2], cy=intr[3],
                                                  c2w=c2w, scene_box=gbox, ray_samples=96)[0], H * W * 96))
        del model
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
