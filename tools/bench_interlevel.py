"""Time the fused interlevel loss (acn_interlevel_loss through interlevel_loss), forward plus backward,
against the torch-op restatement of the same definition (ray_rendering._interlevel_torch: float64 cumsum, two
searchsorted, gathers) on HIP tensors, in one process; and, for orientation, the proposal-guided eval render against the
hierarchical one.

(a) 4096 rays, P = 64 proposal and F = 128 fine samples.  Weights come from compositing a sparse density; t is offset
by 100.  One call is loss.mean() and its backward into w_prop.

Candidates alternated call by call (HIP events around every call, 5 warm-ups, median of 50, twice over -- the
difference of a candidate's two medians is the run-to-run spread).  The fused path stays interlevel_loss's default on
HIP only if it is faster in both rounds by more than the larger round-to-round difference of either candidate.

(b) Orientation only (no criterion: the two renders use different sample sets): eval render_rays of the C2 model
(bench.py's single expert, 4096 rays) at ray_samples = 64, n_importance = 128 with a proposal -- a MetaNGP with 4 of the
main model's 16 hash levels -- against the same call without one, with the HIP kernel launches of one call of each
(torch.profiler's device events).  A second proposal keeps all 16 levels under resolution 128: the fused
field's configuration, whose no-grad density is one launch.

python tools/bench_interlevel.py [--out profiles/bench_interlevel.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from adaptive_city_nerf_amd import interlevel_loss, render_rays  # noqa: E402
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


def histogram(N, S, dev, gen, keep):
    u = (torch.arange(S, device=dev).float()[None, :] + torch.rand(N, S, device=dev, generator=gen)) / S
    t = 100.0 + 2.0 + 30.0 * u
    d = torch.cat([t[:, 1:] - t[:, :-1], t[:, -1:] - t[:, -2:-1]], 1)
    sigma = torch.rand(N, S, device=dev, generator=gen) * 0.4 / keep * (torch.rand(N, S, device=dev, generator=gen)
                                                                         < keep)
    alpha = 1.0 - torch.exp(-sigma * d)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha], -1), -1)[:, :-1]
    return t, (alpha * T).float()


def launches(fn):
    """Device kernel launches of one call (torch.profiler), as {kernel name: count}."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower() and \
                not e.name.lower().startswith(("memcpy", "memset")):
            out[e.name[:80]] = out.get(e.name[:80], 0) + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "bench_interlevel.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_interlevel needs a HIP device"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "HIP events per call, candidates alternated, 5 warm-ups, median of 50, two rounds (ms)"}
    # (a) the loss, forward plus backward
    N, P, F = 4096, 64, 128
    t_prop, w_prop = histogram(N, P, dev, gen, 0.5)
    t_fine, w_fine = histogram(N, F, dev, gen, 0.35)
    wl = w_prop.clone().requires_grad_(True)

    def fused():
        wl.grad = None
        interlevel_loss(t_fine, w_fine, t_prop, wl).backward()
        return wl.grad

    def torch_chain():
        wl.grad = None
        RR._interlevel_torch(t_fine, w_fine, t_prop, wl).mean().backward()
        return wl.grad

    assert RR.FUSED_INTERLEVEL
    gf, gt = fused().clone(), torch_chain().clone()
    dg = float((gf - gt).abs().max() / gt.abs().max())
    cands = {"fused": fused, "torch": torch_chain}
    med = alternate(cands)
    spread = max(abs(v[0] - v[1]) for v in med.values())
    faster = all(med["torch"][r] - med["fused"][r] > spread for r in range(2))
    result["loss_fwd_bwd"] = {"rays": N, "proposal": P, "fine": F, "ms": med, "round_to_round_spread_ms": spread,
                              "max_gradient_difference_over_max_gradient": dg,
                              "fused_faster_in_both_rounds_by_more_than_the_spread": faster}
    result["fused_kept_as_default"] = faster
    print(f"{N} rays, P = {P}, F = {F}: fused {med['fused'][0]:.4f} / {med['fused'][1]:.4f} ms, torch "
          f"{med['torch'][0]:.4f} / {med['torch'][1]:.4f} ms, spread {spread:.4f} ms, fused kept: {faster}; the gradients "
          f"differ by {dg:.1e} of the largest")
    # (b) orientation: the eval render of the C2 model with and without a proposal
    import bench
    from adaptive_city_nerf_amd.meta_ngp import MetaNGP
    model, gbox, scene, sc = bench.build_model(dev, 1)
    model.eval()
    main_enc = (model.submodules[0] if hasattr(model, "submodules") else model).xyz_encoder
    rays = bench.make_rays(scene, gbox, dev, 4096, 7)
    # two proposals: a quarter of the main model's hash levels (hash-grid kernel plus the sigma branch as torch ops),
    # and all 16 levels squeezed under resolution 128 (the fused field's configuration: its density is one launch)
    props, confs = {}, {}
    for tag, levels in (("4 levels", 4), ("16 levels", 16)):
        conf = {"levels": levels, "features_per_level": 2, "log2_hashmap_size": 16, "min_res": 16, "max_res": 128,
                "interpolation": "Linear"}
        torch.manual_seed(1)
        props[tag] = MetaNGP(occ_conf={"use_occ": False}, scene_box=gbox, hidden=64, sigma_depth=2, color_hidden=64,
                             geo_feat_dim=15, color_depth=2, use_sigmoid_rgb=True, hash_enc_conf=conf,
                             dir_encoding="spherical").to(dev).eval()
        confs[tag] = dict(conf, hidden=64, sigma_depth=2, fused_field=bool(props[tag]._fusable))
    with torch.no_grad():
        cands = {f"proposal 64 -> 128, {tag}": (lambda p=p: render_rays(model, rays, ray_samples=64, n_importance=128,
                                                                        proposal=p)) for tag, p in props.items()}
        cands["hierarchical 64 + 128"] = lambda: render_rays(model, rays, ray_samples=64, n_importance=128)
        med = alternate(cands)
        ks = {n: launches(fn) for n, fn in cands.items()}
    result["render_c2_eval_4096_rays"] = {
        "ms": med, "note": "orientation only: different sample sets, not a criterion",
        "main_model": {"levels": int(main_enc.levels), "log2_hashmap_size": int(main_enc.log2_hashmap_size)},
        "proposals": confs,
        "kernel_launches": {n: {"total": sum(v.values()), "kernels": v} for n, v in ks.items()}}
    print("C2 eval render, 4096 rays: " + ", ".join(f"{n} {v[0]:.3f} / {v[1]:.3f} ms ({sum(ks[n].values())} launches)"
                                                     for n, v in med.items()))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
