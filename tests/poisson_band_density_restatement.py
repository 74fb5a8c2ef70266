"""numpy restatement of the banded Poisson call with the density-adaptive splat (reconstruction_amd/csrc/k_poisson_band_density.hip).

Test infrastructure only: the package never imports it.  It builds on poisson_band_restatement (f16) and poisson_density_restatement (f14)
by import and edits neither.  D is the finest depth.  The rules, in DESIGN's numbering:
  1 samples, bricks  f16's: the fine grid o, h, N = 2^D; the coarse grid o, 2 h; the bricks within band_bricks of an occupied one
  2 density          f14's rules 2 and 3 with depth = D: rho_s, w_s, d_s = min(D, max(3, value_s)); once, for both problems below
  3 coarse problem   f14's rules 4 to 6 at depth D - 1 on the same box with the same w_s and d_s clamped to D - 1 -> b_c
  4 fine splat       f14's rule 4 with depth = D; the levels 3..D - 1 are dense, the level D lives on the band (every node a sample touches
                     at level D is active)
  5 combine          W = the levels 3..D - 1 cascaded coarse to fine to level D - 1 with the scales 8^(L - D); on the fine grid
                     U_D = V_D 2^-32 + P(W), P evaluated node by node (prolong_at): x, then y, for the near and the far z-plane, 0.75 near +
                     0.25 far, 0 outside the coarse grid.  V_D = 0 at the inactive nodes, U_D = 0 outside the fine grid
  6 right-hand side  b_f = f7's central differences of U_D in fp64 on the active nodes; a neighbour off the band holds P(W)
  7 guess, solve     f16's (guess, band_solve)
  8 iso              f14's weighted mean on the band's field
  9 extraction, trim f16's
Dense arrays ([k, j, i]) carry the band's fields, as in f16's restatement."""
from __future__ import annotations

import numpy as np

import poisson_band_restatement as pb
import poisson_density_restatement as pd
import poisson_restatement as pr


def resolve_kernel_depth(depth, kernel_depth):
    """0 = D - 2, else 3..D - 1 (the density grid exists in the coarse problem too)"""
    kd = depth - 2 if kernel_depth == 0 else int(kernel_depth)
    assert 3 <= kd <= depth - 1
    return kd


# ---- 5: P at single nodes -------------------------------------------------------------------------------------------------------------------
def prolong_at(A, i, j, k):
    """P(A) at the fine nodes (i, j, k) (integer arrays of one shape, inside the fine grid) for A [..., nc, nc, nc]: the expression of the
    library's cascade, node by node"""
    Ap = np.pad(A, [(0, 0)] * (A.ndim - 3) + [(1, 1)] * 3)                      # Ap[x + 1] = A[x], 0 outside
    two = lambda c: ((c >> 1) + 1, (c >> 1) + 1 + np.where(c & 1, 1, -1))      # the near and the far coarse node
    ci, cj, ck = two(np.asarray(i)), two(np.asarray(j)), two(np.asarray(k))
    y = []
    for c in range(2):
        x0 = 0.75 * Ap[..., ck[c], cj[0], ci[0]] + 0.25 * Ap[..., ck[c], cj[0], ci[1]]
        x1 = 0.75 * Ap[..., ck[c], cj[1], ci[0]] + 0.25 * Ap[..., ck[c], cj[1], ci[1]]
        y.append(0.75 * x0 + 0.25 * x1)
    return 0.75 * y[0] + 0.25 * y[1]


def prolong_everywhere(A):
    """prolong_at at every fine node: [..., 2 nc, 2 nc, 2 nc]"""
    n = 2 * A.shape[-1]
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij", sparse=True)
    return prolong_at(A, i, j, k)


def coarse_levels(V, depth):
    """rule 5's W: the levels 3..depth - 1 of V cascaded to level depth - 1 with the scales 8^(L - depth): fp64 [3, N/2, N/2, N/2]"""
    W = None
    for L in range(pd.L_MIN, depth):
        own = (V[L].astype(np.float64) / pd.FIX) * 8.0 ** (L - depth)
        W = own if W is None else own + pd.prolong(W)
    return W


# ---- 1 to 6 ---------------------------------------------------------------------------------------------------------------------------------
def band_density_rhs(xyz, normals, depth, scale=1.1, band_bricks=1, kernel_depth=0, samples_per_node=2.0, d=None):
    """rules 1 to 6.  d: per-row depths from elsewhere (clamped to 3..D), else rule 2's.  dict: pd.sample_density's keys (p, nh, ok, o, h, kd,
    rho, value, w, d) and occupied, active, bricks, mask, occ (dense, per fine cell), V_D (int64 [3, N, N, N]), W, U (fp64 [3, N, N, N]: U_D on
    the whole fine grid, P(W) off the band), b (dense fp64: read it on the band), b_c (the coarse right-hand side, dense fp64), d_c"""
    kd = resolve_kernel_depth(depth, kernel_depth)
    s = pd.sample_density(xyz, normals, depth, scale, kd, samples_per_node)
    if s is None:
        return None
    if d is not None:
        s["d"] = pd.clamp_depth(np.asarray(d, np.float64).reshape(-1)[s["ok"]], depth)
    p, nh, o, h = s["p"], s["nh"], s["o"], s["h"]
    N = 1 << depth
    occb, act, bricks = pb.bricks_of(p, o, h, depth, band_bricks)
    mask = pb.node_mask(act)
    # 3: the coarse problem
    d_c = np.minimum(s["d"], float(depth - 1))
    Vc, _ = pd.level_splat(p, nh, s["w"], d_c, o, 2.0 * h, depth - 1)
    b_c = pr.rhs(pd.combine(Vc, depth - 1))
    # 4: the fine splat
    V, cnt = pd.level_splat(p, nh, s["w"], s["d"], o, h, depth)
    assert not V[depth][:, ~mask].any() and not cnt[depth][~mask].any()        # every level-D node a sample touches is active
    # 5, 6
    W = coarse_levels(V, depth)
    U = (V[depth].astype(np.float64) / pd.FIX) * 1.0 + prolong_everywhere(W)
    s.update(occupied=occb, active=act, bricks=bricks, mask=mask, occ=pd.occupancy(p, o, h, depth), V_D=V[depth], W=W, U=U, b=pr.rhs(U), b_c=b_c, d_c=d_c,
             cnt=cnt, n_invalid=int((~s["ok"]).sum()))
    return s


def iso_value(chi, p, w, o, h):
    """rule 8: f14's weighted mean; chi dense, read at the samples' (active) nodes"""
    return pd.iso_value(chi, p, w, o, h)


# ---- all of it --------------------------------------------------------------------------------------------------------------------------------
def reconstruct(xyz, normals, depth, scale=1.1, band_bricks=1, trim_cells=0, kernel_depth=0, samples_per_node=2.0, rel_residual=4e-5, max_iterations=200,
                coarse="exact", d=None):
    """Every rule.  coarse: 'exact' = the direct fp64 solution of the coarse system rounded to float32, or a float32 array [N/2]^3."""
    R = band_density_rhs(xyz, normals, depth, scale, band_bricks, kernel_depth, samples_per_node, d)
    if isinstance(coarse, str):
        coarse = pr.solve_exact(R["b_c"]).astype(np.float32)
    g = pb.guess(coarse)
    S = pb.band_solve(R["b"], g, R["mask"], rel_residual, max_iterations)
    chi = S["chi"]
    iso = iso_value(chi, R["p"], R["w"], R["o"], R["h"])
    v0, f0, keys, dkeys = pb.extract_band(chi, iso, R["o"], R["h"], R["bricks"])
    tv, tf = pb.trim_band(v0, f0, R["occ"], R["o"], R["h"], trim_cells, band_bricks)
    R.update(S, g=g, chi_c=coarse, iso=iso, verts0=v0, faces0=f0, keys=keys, dense_keys=dkeys, verts=tv, faces=tf)
    return R


def surface_inside_band(chi, iso, mask):
    """the iso-surface never leaves the band: no lattice edge with an end off the band is crossed (chi holds the guess off the band)"""
    ins = np.asarray(chi, np.float32) < np.float32(iso)
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        if ((ins[a] != ins[b]) & ~(mask[a] & mask[b])).any():
            return False
    return True
