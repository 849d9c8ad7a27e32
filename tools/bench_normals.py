"""Time the fused density-gradient kernel (acn_field_sigma_grad) against the routes it replaces, in one
process: M = 1,048,576 uniform points of the box, one expert at L = 16, F = 2, log2T = 20, Linear and Smoothstep.

Candidates, alternated call by call (HIP events around every call, 5 warm-ups, median of 20, twice over -- the
difference of a candidate's two medians is the run-to-run spread the comparison is read against):
  kernel        ops.field_sigma_grad (weight pack + one launch)
  chain4        the four launches on precomputed unit points: ops.hashgrid_fwd -> ops.mlp_train_fwd ->
                ops.mlp_train_bwd_input (gout = e_sigma) -> ops.hashgrid_bwd_input
  chain         chain4 plus the torch elementwise ops around it (unit coordinates, clamp, pass mask, / extent)
  autograd      MetaNGP.density_and_gradient(create_graph=False) on a frozen model
  autograd_tab  the same with a trainable hash table (autograd then also runs the table scatter)
Then one 800 x 800 x 96 frame through render_normal_image at min_weight 0 and 1e-3, with the share of 32-sample tiles
the gate skips, on the field as initialised (sigma ~ 0.4: nothing occludes) and on a denser one (sigma head bias
+4: the transmittance falls below 1e-3 after a few samples, as behind a surface).

python tools/bench_normals.py [--points M] [--out profiles/bench_normals.json] [--no-frame]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from adaptive_city_nerf_amd import MetaNGP, SceneBox, ops, render_normal_image, render_rays_stratified  # noqa: E402


def expert(interp, dev, log2T=20):
    torch.manual_seed(11)
    conf = {"levels": 16, "features_per_level": 2, "log2_hashmap_size": log2T, "max_res": 4096, "min_res": 16,
            "interpolation": interp}
    m = MetaNGP(occ_conf={"use_occ": False}, scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])),
                hidden=64, sigma_depth=2, color_hidden=64, geo_feat_dim=15, color_depth=2, use_sigmoid_rgb=True,
                hash_enc_conf=conf, dir_encoding="spherical").to(dev)
    with torch.no_grad():
        m.xyz_encoder.hash_table.uniform_(-0.5, 0.5)
    return m.eval().requires_grad_(False)


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


def candidates(m, mt, x):
    enc = m.xyz_encoder
    mn, ext = m.scene_box.min.to(x.device), m.aabb_extent.to(x.device)
    lo, hi = m.enc_eps, 1.0 - m.enc_eps
    ws = [t.detach().contiguous() for t in m._mlp_tensors(None).values()]
    spec = m.expert_spec()
    sh = torch.zeros(x.shape[0], 16, device=x.device)
    gout = torch.zeros(x.shape[0], 4, device=x.device)
    gout[:, 3] = 1.0
    x01 = ((x - mn) / ext).clamp(lo, hi)
    args = (enc._res_host, enc.log2_hashmap_size, 2, enc._interp_code)

    def chain4(p01=x01):
        h0 = ops.hashgrid_fwd(p01, enc.hash_table, *args)
        out, _ = ops.mlp_train_fwd(h0, sh, ws, save=False)
        gh, _ = ops.mlp_train_bwd_input(h0, sh, out, gout, ws, want_sh=False)
        return out, ops.hashgrid_bwd_input(p01, gh, enc.hash_table, *args)

    def chain():
        u = (x - mn) / ext
        out, g = chain4(u.clamp(lo, hi))
        return out[:, 3], g * (((u >= lo) & (u <= hi)).float() / ext)

    return {"kernel": lambda: ops.field_sigma_grad(x, spec), "chain4": chain4, "chain": chain,
            "autograd": lambda: m.density_and_gradient(x), "autograd_tab": lambda: mt.density_and_gradient(x)}


def skipped_share(model, rays, S, min_weight, params, chunk_rays=8192):
    """Share of the 32-sample tiles of render_normals' sigma_gradient calls whose samples are all gated."""
    tiles = skipped = 0
    for a in range(0, rays.shape[0], chunk_rays):
        w = render_rays_stratified(model, rays[a:a + chunk_rays], S, params=params)[2].reshape(-1)
        pad = (-w.numel()) % 32
        off = torch.cat([w <= min_weight, torch.ones(pad, dtype=torch.bool, device=w.device)]).view(-1, 32).all(-1)
        tiles += off.numel()
        skipped += int(off.sum())
    return skipped / max(1, tiles)


def frame(m, dev):
    H = W = 800
    S = 96
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.8]])
    kw = dict(H=H, W=W, fx=700.0, fy=700.0, cx=400.0, cy=400.0, c2w=c2w, scene_box=m.scene_box, ray_samples=S)
    rays, _ = ops.get_rays_image(H, W, 700.0, 700.0, 400.0, 400.0, c2w, m.scene_box.aabb, dev, center_pixels=True,
                                 near_far_override=(None, None), apply_clamp=True)
    dense = dict(m._mlp_tensors(None))
    dense["sigma_head.bias"] = dense["sigma_head.bias"] + 4.0
    rows = []
    for field, params in (("as initialised", None), ("sigma head bias +4", dense)):
        cands = {f"min_weight {mw:g}": (lambda mw=mw: render_normal_image(m, params=params, min_weight=mw, **kw))
                 for mw in (0.0, 1e-3)}
        cands["render_image (no normals)"] = lambda: render_rays_stratified(m, rays, S, params=params,
                                                                            _want_weights=False)
        med = alternate(cands, warmup=1, iters=5, rounds=2)
        for name, v in med.items():
            mw = 1e-3 if name.endswith("0.001") else 0.0
            rows.append({"field": field, "call": name, "ms": v,
                         "tiles_skipped": skipped_share(m, rays, S, mw, params) if name.startswith("min") else None})
            print(f"frame {H}x{W}x{S}, {field:20s} {name:28s} {v[0]:8.2f} / {v[1]:8.2f} ms"
                  + (f"  tiles skipped {rows[-1]['tiles_skipped']:.3f}" if rows[-1]["tiles_skipped"] is not None else ""))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--out", default=str(REPO / "profiles" / "bench_normals.json"))
    ap.add_argument("--no-frame", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_normals needs a HIP device"
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "points": a.points, "precision": ops.TRAIN_MLP_PRECISION,
              "timing": "HIP events per call, candidates alternated, 5 warm-ups, median of 20, two rounds (ms)",
              "interp": {}}
    x = torch.rand(a.points, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 2.0 - 1.0
    for interp in ("Linear", "Smoothstep"):
        m = expert(interp, dev)
        mt = expert(interp, dev)
        mt.xyz_encoder.hash_table.requires_grad_(True)
        cands = candidates(m, mt, x)
        sk, gk = cands["kernel"]()
        sc, gc = cands["chain"]()
        same = bool(torch.equal(sk, sc) and torch.equal(gk, gc))
        med = alternate(cands)
        result["interp"][interp] = {"ms": med, "kernel_equals_chain_bitwise": same}
        for n, v in med.items():
            print(f"{interp:10s} {n:12s} {v[0]:8.3f} / {v[1]:8.3f} ms per {a.points} points (spread {abs(v[0] - v[1]):.3f})")
        k, c = max(med["kernel"]), min(med["chain4"])
        spread = max(abs(v[0] - v[1]) for v in (med["kernel"], med["chain4"]))
        print(f"{interp:10s} kernel (slower round) / chain4 (faster round) = {k / c:.3f}; spread {spread:.3f} ms; "
              f"kernel == chain bit for bit: {same}")
        del m, mt, cands
        torch.cuda.empty_cache()
    if not a.no_frame:
        result["frame_800x800x96"] = frame(expert("Linear", dev), dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
