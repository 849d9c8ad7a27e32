"""Time the frozen-field input backward and a camera-pose step, in one process.

(a) Kernel: acn_mlp_train_bwd_input against acn_mlp_train_bwd_dw of the same build at M = 1,048,576 samples, both
    on the image one forward packed (the _img entry points: no pack launch in either), both returning dL/dh0.  The
    new kernel does a strict subset of the fused backward's work, so it must not be slower.
(b) Pose step: a frozen single-expert container, c2w (device, requires grad) -> get_rays -> render_rays -> loss ->
    backward to c2w.grad, 4096 rays x 64 samples, with _FusedMLPFn.INPUT_GRAD_FUSED on against off (off: the composed
    torch chain for the 14-tensor MLP, the path before the switch existed).  The MLP's share of each step is the
    MLP's forward + input backward timed alone on the step's own 262,144 samples (hash and SH features as leaves)
    over the step time.

HIP events around every single call, median of 20 after 5 warm-ups; the two variants of a pair alternate.  Prints a
table and writes profiles/bench_pose_grad.json (or --out).

python tools/bench_pose_grad.py [--samples M] [--rays N] [--ray-samples S] [--precision fp16x3|fp32] [--out PATH]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import bench  # noqa: E402
from adaptive_city_nerf_amd import ops, render_rays  # noqa: E402
from adaptive_city_nerf_amd._lib import check, ptr, stream_of  # noqa: E402
from adaptive_city_nerf_amd.meta_ngp import _FusedMLPFn  # noqa: E402
from adaptive_city_nerf_amd.ray_sampling import get_rays  # noqa: E402


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


def kernel_pair(sub, M, precision, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    ws = [t.detach().contiguous() for t in sub._mlp_tensors(None).values()]
    h0 = (torch.rand(M, 32, device=dev, generator=gen) - 0.5) * 2
    sh = (torch.rand(M, 16, device=dev, generator=gen) - 0.5) * 2
    gout = torch.randn(M, 4, device=dev, generator=gen)
    out, _, img = ops.mlp_train_fwd(h0, sh, ws, save=False, precision=precision, return_img=True)
    gh, gsh = torch.empty(M, 32, device=dev), torch.empty(M, 16, device=dev)
    dw = torch.empty(ops.MLP_DW_FLOATS, device=dev)
    wsp = torch.empty(int(ops.mlp_fn("acn_mlp_dw_workspace_bytes", precision)()), dtype=torch.uint8, device=dev)
    f_in, f_dw = ops.mlp_fn("acn_mlp_train_bwd_input_img", precision), ops.mlp_fn("acn_mlp_train_bwd_dw_img", precision)
    st = stream_of(h0)
    # the C ABI directly, outputs allocated once: the host work between the two events is one ctypes call
    t_in, t_in_h0, t_dw = alternate_ms([
        lambda: check(f_in(ptr(h0), ptr(sh), ptr(out), ptr(gout), M, ptr(img), ptr(gh), ptr(gsh), st), "bwd_input"),
        lambda: check(f_in(ptr(h0), ptr(sh), ptr(out), ptr(gout), M, ptr(img), ptr(gh), None, st), "bwd_input"),
        lambda: check(f_dw(ptr(h0), ptr(sh), ptr(out), ptr(gout), M, ptr(img), ptr(dw), ptr(gh), ptr(wsp), st), "bwd_dw")])
    return {"M": M, "precision": precision, "bwd_input_us": t_in * 1e3, "bwd_input_h0_only_us": t_in_h0 * 1e3,
            "bwd_dw_us": t_dw * 1e3, "bwd_input_over_bwd_dw": t_in / t_dw}


def composed_mlp(sub, h0, sh):
    """MetaNGP.density + color on given features: the torch chain INPUT_GRAD_FUSED = False runs."""
    h = sub.sigma_trunk(h0)
    sigma = sub.sigma_act(sub.sigma_head(h))
    rgb = sub.rgb_act(sub.color_mlp(torch.cat([sub.geo_head(h), sh], dim=-1)))
    return torch.cat([rgb, sigma], dim=-1)


def pose_step(model, gbox, scene, N, S, dev):
    sub = model.submodules[0]
    H, W, intr, cam = bench.frame_camera(scene)
    psf = scene["pose_scale_factor"]
    _, valid = ops.get_rays_image(H, W, *intr, cam, gbox.aabb, dev, near_far_override=(0.0, 100000 / psf))
    vi = torch.nonzero(valid).squeeze(1).cpu()
    sel = vi[torch.randperm(vi.numel(), generator=torch.Generator().manual_seed(7))[:N]].to(dev)
    dirs = ops.ray_directions(H, W, *intr, True, dev).view(-1, 3)[sel].contiguous()
    c2w = cam[:3, :4].float().to(dev).requires_grad_()
    gen = torch.Generator(device=dev).manual_seed(1)
    wr, wd = torch.randn(N, 3, device=dev, generator=gen), torch.randn(N, device=dev, generator=gen)

    def step(on):
        def run():
            _FusedMLPFn.INPUT_GRAD_FUSED = on
            c2w.grad = None
            rays = get_rays(dirs, c2w, scene_box=gbox)
            rgb, depth, _, _ = render_rays(model, rays, ray_samples=S)
            ((rgb * wr).sum() + (depth * wd).sum()).backward()
        return run

    # the MLP alone on the step's sample count (features as leaves)
    M = N * S
    h0 = ((torch.rand(M, 32, device=dev, generator=gen) - 0.5) * 2).requires_grad_()
    sh = ((torch.rand(M, 16, device=dev, generator=gen) - 0.5) * 2).requires_grad_()
    gout = torch.randn(M, 4, device=dev, generator=gen)
    ws = [t.contiguous() for t in sub._mlp_tensors(None).values()]

    def mlp_fused():
        _FusedMLPFn.INPUT_GRAD_FUSED = True
        torch.autograd.grad(_FusedMLPFn.apply(h0, sh, *ws), [h0, sh], gout)

    def mlp_composed():
        torch.autograd.grad(composed_mlp(sub, h0, sh), [h0, sh], gout)

    try:
        t_on, t_off = alternate_ms([step(True), step(False)])
        grad_on = (step(True)(), c2w.grad.clone())[1]
        grad_off = (step(False)(), c2w.grad.clone())[1]
        m_on, m_off = alternate_ms([mlp_fused, mlp_composed])
    finally:
        _FusedMLPFn.INPUT_GRAD_FUSED = True
    diff = float((grad_on - grad_off).abs().max() / grad_off.abs().max())
    return {"rays": N, "ray_samples": S, "step_fused_ms": t_on, "step_composed_ms": t_off,
            "speedup": t_off / t_on, "mlp_fused_ms": m_on, "mlp_composed_ms": m_off,
            "mlp_share_fused": m_on / t_on, "mlp_share_composed": m_off / t_off,
            "c2w_grad_max_rel_diff": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--ray-samples", type=int, default=64)
    ap.add_argument("--precision", default="fp16x3", choices=("fp16x3", "fp32"))
    ap.add_argument("--out", default=str(REPO / "profiles" / "bench_pose_grad.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pose_grad.py measures on a HIP device"
    dev = torch.device("cuda", 0)
    ops.set_train_mlp_precision(a.precision)
    model, gbox, scene, _ = bench.build_model(dev, 1)
    model.requires_grad_(False)
    res = {"device": torch.cuda.get_device_name(0), "method": "HIP events per call, median of 20 after 5 warm-ups, "
           "variants alternating", "kernel": kernel_pair(model.submodules[0], a.samples, a.precision, dev),
           "pose_step": pose_step(model, gbox, scene, a.rays, a.ray_samples, dev)}
    k, p = res["kernel"], res["pose_step"]
    print(f"(a) M = {k['M']} ({k['precision']}): acn_mlp_train_bwd_input {k['bwd_input_us']:.1f} us "
          f"(gh0 only {k['bwd_input_h0_only_us']:.1f} us), acn_mlp_train_bwd_dw {k['bwd_dw_us']:.1f} us, "
          f"ratio {k['bwd_input_over_bwd_dw']:.3f}")
    print(f"(b) pose step {p['rays']} rays x {p['ray_samples']}: fused {p['step_fused_ms']:.3f} ms (MLP alone "
          f"{p['mlp_fused_ms']:.3f} ms, {100 * p['mlp_share_fused']:.0f}%), composed {p['step_composed_ms']:.3f} ms "
          f"(MLP alone {p['mlp_composed_ms']:.3f} ms, {100 * p['mlp_share_composed']:.0f}%), speed-up "
          f"{p['speedup']:.2f}x; max|c2w.grad fused - composed| / max = {p['c2w_grad_max_rel_diff']:.2e}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
