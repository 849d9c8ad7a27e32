"""Time the fused render at caller-supplied depths (acn_render_depths_fwd through render_rays_at)
against the composed chain it replaces in the fine pass of render_rays_hierarchical (the (N * S, 6) point table, the
field forward, the background, volume_render), in one process.

Workload: the C2 model (bench.py's single expert) and 4096 rays in eval mode.
 (a) the fine pass alone at S = 192 and 384, on the merged depths of a 64 + 128 and a 256 + 128 resampling:
     render_rays_at (fused) against the chain;
 (b) the whole call: render_rays(ray_samples=64, n_importance=128) with FUSED_FINE_RENDER on and off, and the
     256-sample stratified render_rays beside it.
For the record only: (a) at 64 + 128 on the K = 4 container (bench.py's c3 model).

Candidates alternated call by call (HIP events around every call, 5 warm-ups, median of 50, twice over -- the
difference of a candidate's two medians is its run-to-run spread).  The fused fine pass is the default when its slower
round beats the chain's faster round by more than the larger of the two candidates' round-to-round differences in (a)
at both sizes, and it is not slower in (b).

python tools/bench_render_depths.py [--out profiles/bench_render_depths.json]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))
from adaptive_city_nerf_amd import render_rays, render_rays_at, render_rays_stratified, sample_pdf  # noqa: E402
from adaptive_city_nerf_amd import ray_rendering as RR  # noqa: E402
from bench_resample import alternate  # noqa: E402


def chain(model, rays, t):
    """The fine pass as render_rays_hierarchical composes it with FUSED_FINE_RENDER off."""
    N, S = t.shape
    rgb_sigma = model(RR._points6(rays, t), params=None).view(N, S, 4)
    bg = RR._get_bg_rgb(model, rays[:, 3:6], None, rgb_sigma, N=N, bg_color_default="white")
    return RR.volume_render(rgb_sigma, t, bg_rgb=bg)


def merged_depths(model, rays, S, F):
    coarse = render_rays_stratified(model, rays, S, return_t_vals=True)
    return sample_pdf(coarse[4], coarse[2], F, return_merged=True)[1]


def spread(v):
    return abs(v[0] - v[1])


def fine_pass(model, rays, S, F):
    t = merged_depths(model, rays, S, F)
    assert RR._fused_depths(model, rays, t, None, None, "white") is not None
    cands = {"fused": lambda: render_rays_at(model, rays, t), "chain": lambda: chain(model, rays, t)}
    gf, gc = cands["fused"](), cands["chain"]()
    err = {n: float((a - b).abs().max()) for n, a, b in zip(("rgb", "depth", "weights", "acc"), gf, gc)}
    med = alternate(cands)
    margin = min(med["chain"]) - max(med["fused"])
    need = max(spread(med["fused"]), spread(med["chain"]))
    return {"rays": rays.shape[0], "coarse": S, "fine": F, "ms": med, "max_abs_difference": err,
            "chain_faster_round_minus_fused_slower_round_ms": margin, "larger_round_to_round_difference_ms": need,
            "fused_wins": margin > need}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "bench_render_depths.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render_depths needs a HIP device"
    import bench
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "HIP events per call, candidates alternated, 5 warm-ups, median of 50, two rounds (ms)",
              "fine_pass_c2": {}}
    model, gbox, scene, sc = bench.build_model(dev, 1)
    model.eval()
    rays = bench.make_rays(scene, gbox, dev, 4096, 7)
    wins = True
    with torch.no_grad():
        for S, F in ((64, 128), (256, 128)):
            r = fine_pass(model, rays, S, F)
            result["fine_pass_c2"][f"{S} + {F}"] = r
            wins = wins and r["fused_wins"]
            m = r["ms"]
            print(f"(a) C2 fine pass, 4096 rays x {S + F}: fused {m['fused'][0]:.4f} / {m['fused'][1]:.4f} ms, chain "
                  f"{m['chain'][0]:.4f} / {m['chain'][1]:.4f} ms; margin {r['chain_faster_round_minus_fused_slower_round_ms']:.4f}"
                  f" ms against a spread of {r['larger_round_to_round_difference_ms']:.4f} ms; max differences "
                  f"{r['max_abs_difference']}")

        def whole(flag):
            def run():
                prev = RR.FUSED_FINE_RENDER
                RR.FUSED_FINE_RENDER = flag
                try:
                    return render_rays(model, rays, ray_samples=64, n_importance=128)
                finally:
                    RR.FUSED_FINE_RENDER = prev
            return run

        cands = {"hierarchical 64 + 128, fused fine pass": whole(True),
                 "hierarchical 64 + 128, chain": whole(False),
                 "stratified 256": lambda: render_rays(model, rays, ray_samples=256)}
        med = alternate(cands)
        on, off = med["hierarchical 64 + 128, fused fine pass"], med["hierarchical 64 + 128, chain"]
        not_slower = sum(on) <= sum(off)   # the mean of the two rounds
        result["whole_call_c2"] = {"ms": med, "fused_not_slower": not_slower}
        print("(b) C2 render_rays, 4096 rays: " + ", ".join(f"{n} {v[0]:.4f} / {v[1]:.4f} ms" for n, v in med.items()))
        result["fused_fine_render_default"] = bool(wins and not_slower)
        print(f"FUSED_FINE_RENDER default by this run: {result['fused_fine_render_default']}")
        # for the record: the K = 4 container
        m4, gbox4, scene4, sc4 = bench.build_model(dev, 4)
        m4.eval()
        rays4 = bench.make_rays(scene4, gbox4, dev, 4096, 7)
        r = fine_pass(m4, rays4, 64, 128)
        result["fine_pass_k4_for_the_record"] = r
        m = r["ms"]
        print(f"K = 4 fine pass, 4096 rays x 192: fused {m['fused'][0]:.4f} / {m['fused'][1]:.4f} ms, chain "
              f"{m['chain'][0]:.4f} / {m['chain'][1]:.4f} ms")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
