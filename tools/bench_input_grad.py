"""Time the hash-grid input-gradient kernel (acn_hashgrid_bwd_input) and its double backward
(acn_hashgrid_bwd_input_bwd, acn_hashgrid_bwd_input_bwd_table) against the forward (acn_hashgrid_fwd)
and the table backward (acn_hashgrid_bwd) of the same build, in one process: M = 1,048,576 uniform points (C2's
sample count), L = 16, F = 2, log2T = 20, Linear.

HIP events around every single launch, median of 20 after 5 warm-ups.  Both kernels gather the
same 8 rows per (point, level); the bytes/s figures are over the algorithmic traffic per point: 16 levels x 8 rows x
8 B = 1024 B of table rows, 128 B of features (written by the forward, read as grad_out by the backward) and 24 B
of points and point gradients.  There is no gate: the forward is the yardstick of the two gather kernels (the
double backward reads grad_out and the 12-B cotangent and writes 128 B + 12 B more than the first backward; its line
counts those), the float-atomic acn_hashgrid_bwd that of the scatter (the same 16 x 8 x 2 atomics per point).

python tools/bench_input_grad.py [--interp 1|2] [--points M]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from adaptive_city_nerf_amd._lib import check, lib, ptr, stream_of  # noqa: E402
from oracle import oracle as O  # noqa: E402


def median_ms(fn, warmup=5, iters=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--interp", type=int, default=1, choices=(1, 2))
    ap.add_argument("--points", type=int, default=1 << 20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L, F, log2T, M = 16, 2, 20, a.points
    res = O.level_resolutions(L, 16, 4096).tolist()
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(M, 3, device=dev, generator=gen)
    table = (torch.rand(L << log2T, F, device=dev, generator=gen) - 0.5)
    g = torch.randn(M, L * F, device=dev, generator=gen)
    # the C ABI directly, outputs allocated once: the host work between the two events is one ctypes call
    import ctypes
    out, gx = torch.empty(M, L * F, device=dev), torch.empty(M, 3, device=dev)
    r32, st = (ctypes.c_int32 * L)(*res), stream_of(x)
    fwd = median_ms(lambda: check(lib().acn_hashgrid_fwd(ptr(x), M, ptr(table), r32, L, log2T, F, a.interp, ptr(out),
                                                         st), "acn_hashgrid_fwd"))
    bwd = median_ms(lambda: check(lib().acn_hashgrid_bwd_input(ptr(x), M, ptr(g), ptr(table), r32, L, log2T, F,
                                                               a.interp, ptr(gx), st), "acn_hashgrid_bwd_input"))
    v = torch.randn(M, 3, device=dev, generator=gen)
    gg, gx2 = torch.empty(M, L * F, device=dev), torch.empty(M, 3, device=dev)
    gt = torch.zeros(L << log2T, F, device=dev)     # the scatters accumulate: values grow, the work does not change
    bwd2 = median_ms(lambda: check(lib().acn_hashgrid_bwd_input_bwd(ptr(x), M, ptr(g), ptr(v), ptr(table), r32, L, log2T,
                                                                    F, a.interp, ptr(gg), ptr(gx2), st),
                                   "acn_hashgrid_bwd_input_bwd"))
    scat = median_ms(lambda: check(lib().acn_hashgrid_bwd(ptr(x), M, ptr(g), r32, L, log2T, F, a.interp, ptr(gt), st),
                                   "acn_hashgrid_bwd"))
    scat2 = median_ms(lambda: check(lib().acn_hashgrid_bwd_input_bwd_table(ptr(x), M, ptr(g), ptr(v), r32, L, log2T, F,
                                                                          a.interp, ptr(gt), st),
                                    "acn_hashgrid_bwd_input_bwd_table"))
    per_point = 1024 + 128 + 24
    for name, ms, extra in (("acn_hashgrid_fwd", fwd, 0), ("acn_hashgrid_bwd_input", bwd, 0),
                            ("acn_hashgrid_bwd_input_bwd", bwd2, 128 + 24)):
        print(f"{name:32s} {M} pts x {L} levels, interp {a.interp}: {ms * 1e3:8.1f} us  "
              f"{M * (per_point + extra) / (ms * 1e-3) / 1e12:6.3f} TB/s algorithmic")
    for name, ms in (("acn_hashgrid_bwd", scat), ("acn_hashgrid_bwd_input_bwd_table", scat2)):
        print(f"{name:32s} {M} pts x {L} levels, interp {a.interp}: {ms * 1e3:8.1f} us  "
              f"{M * 1024 / (ms * 1e-3) / 1e12:6.3f} TB/s of added bytes")
    print(f"bwd_input / fwd = {bwd / fwd:.3f}")
    print(f"bwd_input_bwd / fwd = {bwd2 / fwd:.3f}")
    print(f"bwd_input_bwd_table / bwd = {scat2 / scat:.3f}")


if __name__ == "__main__":
    main()
