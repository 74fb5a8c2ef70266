"""numpy restatement of the density-adaptive splat of the Poisson surface (reconstruction_amd/csrc/k_poisson_density.hip).

Test infrastructure only: the package never imports it.  It builds on poisson_restatement (f7) and meshtrim_restatement (f11) and edits
neither.  The rules, in DESIGN's numbering:
  1 samples, grids  f7's valid samples and f7's box o, side.  Level L has N_L = 2^L nodes per axis at o + (i + 1/2) h_L, h_L = side / N_L;
                    levels L_MIN = 3 .. depth.
  2 density         rho_s = f11's count splat on 2^kernel_depth nodes of all valid samples, read back at the sample's own position
                    (meshtrim_restatement.density); value_s = max(0, kernel_depth + 1/2 log2(rho_s / samples_per_node)).
  3 weight, depth   w_s = min(1, 1 / (64 rho_s)); d_s = min(depth, max(3, value_s)); lo_s = floor(d_s), fr_s = d_s - lo_s.
  4 splat           at level lo_s with alpha = (1 - fr_s) w_s and, when lo_s < depth, at lo_s + 1 with alpha = fr_s w_s:
                    V_L[a](node) += llrint((wt (alpha n^_a)) 2^32), f7's trilinear weights on that level's grid, outside dropped; int64.
  5 combine         U_3 = V_3 2^-32 8^(3 - depth); U_L = V_L 2^-32 8^(L - depth) + P(U_{L-1}); P = cell-centred trilinear prolongation, one
                    axis at a time in the order x, y, z: fine j takes 0.75 A[j >> 1] + 0.25 A[(j >> 1) + (1 if j & 1 else -1)], 0 outside.
  6 right-hand side f7's central differences of U_depth in fp64 (poisson_restatement.rhs).
  7 iso             sum w_s chi(p_s) / sum w_s over the valid samples, chi(p_s) = f7's trilinear interpolation.
  8 extraction      f7's (poisson_restatement.extract / trim).
The arrays are indexed [k, j, i] (C order = the linear index), as in poisson_restatement."""
from __future__ import annotations

import numpy as np

import meshtrim_restatement as mt
import poisson_restatement as pr

L_MIN = 3
FIX = 4294967296.0   # 2^32


def sample_density(xyz, normals, depth, scale=1.1, kernel_depth=0, samples_per_node=2.0):
    """rules 1-3 at the valid samples: dict p, nh, ok (mask over the rows), o, h (the finest step), kd, rho, value, w, d"""
    p, nh, ok = pr.valid_samples(xyz, normals)
    g = pr.make_grid(p, depth, scale)
    if g is None:
        return None
    o, h = g
    kd = mt.resolve_kernel_depth(depth, kernel_depth)
    # the sample's own position is a float32 point: f11's rule at it, with all valid samples as the cloud
    rho, value, _ = mt.density(xyz, normals, p.astype(np.float32), depth, scale, kd, samples_per_node)
    w = np.minimum(1.0, 1.0 / (64.0 * rho))
    return dict(p=p, nh=nh, ok=ok, o=o, h=h, kd=kd, rho=rho, value=value, w=w, d=clamp_depth(value, depth))


def clamp_depth(d, depth):
    return np.minimum(float(depth), np.maximum(float(L_MIN), np.asarray(d, np.float64)))


def level_step(h, depth, L):
    """h_L = side / 2^L (side = h 2^depth; the powers of two are exact both ways)"""
    return (h * float(1 << depth)) / float(1 << L)


def level_splat(p, nh, w, d, o, h, depth):
    """rule 4: {L: V_L int64 [3, N_L, N_L, N_L]} and {L: cnt_L int64 [N_L, N_L, N_L]} = contributions per node"""
    lo = np.floor(d)
    fr = d - lo
    lo = lo.astype(np.int64)
    V, cnt = {}, {}
    for L in range(L_MIN, depth + 1):
        N = 1 << L
        V[L] = np.zeros((3, N * N * N), np.int64)
        cnt[L] = np.zeros(N * N * N, np.int64)
        for sel, alpha in ((lo == L, (1.0 - fr) * w), ((lo == L - 1) & (lo < depth), fr * w)):
            if not sel.any():
                continue
            idx, wt, inside = pr._trilinear(p[sel], o, level_step(h, depth, L), N)
            lin = idx[..., 0] + N * (idx[..., 1] + N * idx[..., 2])
            an = alpha[sel][:, None] * nh[sel]                                   # alpha n^_a
            for a in range(3):
                q = np.rint((wt * an[:, a:a + 1]) * FIX).astype(np.int64)
                np.add.at(V[L][a], lin[inside], q[inside])
            np.add.at(cnt[L], lin[inside], 1)
        V[L] = V[L].reshape(3, N, N, N)
        cnt[L] = cnt[L].reshape(N, N, N)
    return V, cnt


def _prolong_axis(A, axis):
    n = A.shape[axis]
    P = np.pad(A, [(1, 1) if a == axis else (0, 0) for a in range(A.ndim)])
    j = np.arange(2 * n)
    near = np.take(P, (j >> 1) + 1, axis)
    far = np.take(P, (j >> 1) + 1 + np.where(j & 1, 1, -1), axis)
    return 0.75 * near + 0.25 * far


def prolong(A):
    """P of rule 5 on the last three axes of A ([..., k, j, i]): x, then y, then z"""
    nd = A.ndim
    return _prolong_axis(_prolong_axis(_prolong_axis(A, nd - 1), nd - 2), nd - 3)


def combine(V, depth):
    """rule 5: U_depth fp64 [3, N, N, N]"""
    U = None
    for L in range(L_MIN, depth + 1):
        own = (V[L].astype(np.float64) / FIX) * 8.0 ** (L - depth)
        U = own if U is None else own + prolong(U)
    return U


def occupancy(p, o, h, depth):
    N = 1 << depth
    c = np.clip(np.floor((p - o) / h).astype(np.int64), 0, N - 1)
    occ = np.zeros(N * N * N, np.uint8)
    occ[c[:, 0] + N * (c[:, 1] + N * c[:, 2])] = 1
    return occ.reshape(N, N, N)


def expand(values, ok, fill=0.0):
    """per-valid-sample values as one per row, `fill` at the rows that take no part"""
    out = np.full(len(ok), fill, np.float64)
    out[ok] = values
    return out


def rhs_of(xyz, normals, depth, scale=1.1, kernel_depth=0, samples_per_node=2.0, d=None):
    """rules 1-6.  d: per-row depths from elsewhere (clamped as rule 3 says), else this restatement's.  dict: sample_density's keys and
    V, cnt, U, b, occ"""
    s = sample_density(xyz, normals, depth, scale, kernel_depth, samples_per_node)
    if s is None:
        return None
    if d is not None:
        s["d"] = clamp_depth(np.asarray(d, np.float64).reshape(-1)[s["ok"]], depth)
    V, cnt = level_splat(s["p"], s["nh"], s["w"], s["d"], s["o"], s["h"], depth)
    U = combine(V, depth)
    s.update(V=V, cnt=cnt, U=U, b=pr.rhs(U), occ=occupancy(s["p"], s["o"], s["h"], depth))
    return s


def chi_at_samples(chi, p, o, h):
    """f7's item 6 per sample: the eight terms in the corner order dz, dy, dx"""
    N = chi.shape[0]
    idx, wt, inside = pr._trilinear(p, o, h, N)
    idx = np.clip(idx, 0, N - 1)
    c = np.asarray(chi, np.float64)[idx[..., 2], idx[..., 1], idx[..., 0]]
    acc = np.zeros(len(p))
    for k in range(8):
        acc = acc + np.where(inside[:, k], wt[:, k] * c[:, k], 0.0)
    return acc


def iso_value(chi, p, w, o, h):
    """rule 7"""
    return float((w * chi_at_samples(chi, p, o, h)).sum() / w.sum())


def reconstruct(xyz, normals, depth, scale=1.1, kernel_depth=0, samples_per_node=2.0, rel_residual=1e-10, trim_cells=0):
    """All eight rules with poisson_restatement's solver and extraction: rhs_of's keys and chi, chi32, iso, verts, faces"""
    s = rhs_of(xyz, normals, depth, scale, kernel_depth, samples_per_node)
    if s is None:
        return dict(verts=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32), o=None, h=0.0)
    chi, res = pr.solve(s["b"], rel_residual)
    iso = iso_value(chi, s["p"], s["w"], s["o"], s["h"])
    chi32 = chi.astype(np.float32)
    verts, faces, keys = pr.extract(chi32, iso, s["o"], s["h"])
    tv, tf = pr.trim(verts, faces, s["occ"], s["o"], s["h"], trim_cells)
    s.update(chi=chi, chi32=chi32, iso=iso, residual=res, verts=tv, faces=tf, verts0=verts, faces0=faces, keys=keys)
    return s


# ---- inputs and figures the tests share -----------------------------------------------------------------------------------------------------
def thinned_sphere(keep_upper, n=60000, seed=5, noise=0.3):
    """f7's sphere from n directions of default_rng(seed); the lower hemisphere whole, the upper thinned to the share keep_upper"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    keep = (d[:, 2] < 0.0) | (rng.uniform(size=n) < keep_upper)
    r = pr.SPHERE_R + noise * rng.normal(size=n)
    return pr._with_normals((pr.SPHERE_C + d * r[:, None])[keep], d[keep])


SETUPS = {"A": dict(depth=6, keep_upper=0.03), "B": dict(depth=5, keep_upper=0.10)}


def setup_samples(name):
    return thinned_sphere(SETUPS[name]["keep_upper"])


def side_errors(verts, h):
    """(max, rms) radial error in h of the vertices with z >= c_z + 5 (the sparse side), the same with z <= c_z - 5 (the dense side)"""
    v = np.asarray(verts, np.float64)
    e = pr.radial_error_h(v, h)
    out = []
    for m in (v[:, 2] >= pr.SPHERE_C[2] + 5.0, v[:, 2] <= pr.SPHERE_C[2] - 5.0):
        out.append((float(e[m].max()), float(np.sqrt((e[m] ** 2).mean()))) if m.any() else (float("inf"), float("inf")))
    return out[0], out[1]
