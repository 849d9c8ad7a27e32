"""Reference of the second-order tests: the double backward of the hash grid's point gradient written out from its
formulas, in float64, on CPU or GPU tensors.

With u the raw weights of a level (from the float32 product x * res, as input_grad_ref.hashgrid(weights="fp32")
takes them), w = S(u), c_b = prod_a (b_a ? w_a : 1 - w_a), sgn_a = b_a ? +1 : -1, D_ab = d c_b / d w_a, T_b the
corner's table row and V_b = sum_f g_lf T_bf, the first backward is gx_a = sum_l r S'(u_a) sum_b D_ab V_b, and for a
cotangent v (M,3) the derivatives of sum_a v_a gx_a are

  gg[l,f]    = sum_b k_b T_bf,                 k_b = sum_a v_a r S'(u_a) D_ab
  gT[row_b,f] += k_b g_lf
  gx2[e]     = sum_l r^2 sum_b V_b (v_e S''(u_e) D_eb + sum_{a != e} v_a S'(u_a) S'(u_e) sgn_a sgn_e W_o(b_o)),
               o the third axis, W_o(b_o) its weight.

double_backward returns these with their scales: B_gg, B_x and B_row are the same sums with every term (one per
corner, axis and feature) replaced by its absolute value, n_row the number of (point, corner) contributions of a
table row.  Nearest: zeros everywhere, n_row = 0.
"""
import itertools

import torch

from input_grad_ref import P1, P2


def double_backward(x, g, v, table, res, log2T, interp):
    dt = torch.float64
    dev = x.device
    M, L, F = x.shape[0], len(res), table.shape[1]
    x32 = x.detach().to(torch.float32)
    g, v, table = g.detach().to(dt), v.detach().to(dt), table.detach().to(dt)
    out = {"gg": torch.zeros(M, L * F, dtype=dt, device=dev), "gx2": torch.zeros(M, 3, dtype=dt, device=dev),
           "gT": torch.zeros_like(table)}
    out["B_gg"], out["B_x"], out["B_row"] = (torch.zeros_like(out[k]) for k in ("gg", "gx2", "gT"))
    out["n_row"] = torch.zeros(table.shape[0], dtype=torch.int64, device=dev)
    if interp == 0:
        return out
    one = torch.ones(M, dtype=torch.int64, device=dev)
    for l in range(L):
        r = float(res[l])
        s32 = x32 * torch.tensor(r, dtype=torch.float32, device=dev)
        fl = torch.floor(s32)
        u = (s32 - fl).to(dt)
        i0 = fl.to(torch.int64)
        q = 1.0 - u                      # exact: u is a float32 value
        if interp == 2:                  # 1 - S(u) = S(1 - u), free of the cancellation next to w = 1
            w, wc, s1, s2 = (u * u) * (3.0 - 2.0 * u), (q * q) * (3.0 - 2.0 * q), 6.0 * u * q, 6.0 - 12.0 * u
        else:
            w, wc, s1, s2 = u, q, torch.ones_like(u), torch.zeros_like(u)
        sl = slice(l * F, (l + 1) * F)
        gl = g[:, sl]
        for bits in itertools.product((0, 1), repeat=3):
            W = [w[:, a] if bits[a] else wc[:, a] for a in range(3)]
            sg = [1.0 if bits[a] else -1.0 for a in range(3)]
            h = ((i0[:, 0] + bits[0]) ^ ((i0[:, 1] + bits[1]) * P1) ^ ((i0[:, 2] + bits[2]) * P2)) & ((1 << log2T) - 1)
            idx = (l << log2T) + h
            T = table[idx]
            V, Vabs = (gl * T).sum(-1), (gl.abs() * T.abs()).sum(-1)
            D = [sg[0] * W[1] * W[2], W[0] * sg[1] * W[2], W[0] * W[1] * sg[2]]
            kt = [v[:, a] * r * s1[:, a] * D[a] for a in range(3)]
            k, kabs = kt[0] + kt[1] + kt[2], kt[0].abs() + kt[1].abs() + kt[2].abs()
            out["gg"][:, sl] += k[:, None] * T
            out["B_gg"][:, sl] += kabs[:, None] * T.abs()
            out["gT"].index_add_(0, idx, k[:, None] * gl)
            out["B_row"].index_add_(0, idx, kabs[:, None] * gl.abs())
            out["n_row"].index_add_(0, idx, one)
            for e in range(3):
                term = v[:, e] * s2[:, e] * D[e]
                tabs = term.abs()
                for a in range(3):
                    if a != e:
                        c = v[:, a] * s1[:, a] * s1[:, e] * (sg[a] * sg[e]) * W[3 - a - e]
                        term = term + c
                        tabs = tabs + c.abs()
                out["gx2"][:, e] += (r * r) * V * term
                out["B_x"][:, e] += (r * r) * Vabs * tabs
    return out
