"""The mesh colouring of DESIGN.md 9 (f9) restated in numpy, written from the definitions (not from csrc/k_meshcolor.hip): texture_color
(CCloudOptimization.cpp:400-421, line by line), the camera centre, the vertex normals, the depth buffer and the colours.  float32 where the
definitions say float, fp64 elsewhere; every sum in the stated order (numpy's elementwise operations are IEEE basic operations, never fused).
The GPU tests hold the kernels to these functions exactly."""
import numpy as np

GREY = 127
INT_LO, INT_HI = -2147483649.0, 2147483648.0


def dot3(a0, a1, a2, b0, b1, b2):
    """Eigen's 3-vector reduction as the project fixes it: (a0 b0 + a1 b1) + a2 b2"""
    return (a0 * b0 + a1 * b1) + a2 * b2


def rt_of(P):
    """R, T: the float casts of P's columns (cv2eigen of P, CCloudOptimization.cpp:68-71)"""
    P = np.asarray(P, np.float64).reshape(3, 4)
    return P[:, :3].astype(np.float32), P[:, 3].astype(np.float32)


def project(P, xyz):
    """current_imgPt = current_R * current_point + current_T (:406), float: q [n, 3]"""
    R, T = rt_of(P)
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([dot3(R[k, 0], R[k, 1], R[k, 2], p[:, 0], p[:, 1], p[:, 2]) + T[k] for k in range(3)], axis=1).astype(np.float32)


def ROUND(t):
    """#define ROUND(x) (int)((x) + 0.5) on a float quotient (SharedInclude.h:48): the double sum truncated; ok = False where C leaves the
    conversion undefined (not finite, outside int)"""
    with np.errstate(all="ignore"):
        v = np.asarray(t, np.float32).astype(np.float64) + 0.5
        ok = (v > INT_LO) & (v < INT_HI)
        return np.where(ok, np.trunc(np.where(ok, v, 0.0)), 0.0).astype(np.int64), ok


def pixel_of(q, W, H):
    """int current_x = ROUND(q0 / q2), current_y = ROUND(q1 / q2) (:407-408) and the test of :409-410: (x, y, inside)"""
    with np.errstate(all="ignore"):
        x, okx = ROUND(q[:, 0] / q[:, 2])
        y, oky = ROUND(q[:, 1] / q[:, 2])
    inside = okx & oky & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    return x, y, inside


def texture_color(xyz, P, image):
    """texture_color (:400-421) over an array: rgb uint8 [n, 3]"""
    img = np.asarray(image, np.uint8)
    H, W = img.shape[:2]
    q = project(P, xyz)
    x, y, inside = pixel_of(q, W, H)
    rgb = np.full((len(q), 3), GREY, np.uint8)              # :412-414
    px = img[y[inside], x[inside]]                          # base_ptr = current_img + (width * y + x) * 3
    rgb[inside, 2] = px[:, 0]                               # :418-420
    rgb[inside, 1] = px[:, 1]
    rgb[inside, 0] = px[:, 2]
    return rgb


def det3(a, b, c):
    """the determinant of the matrix whose columns are a, b, c, expanded along the first column"""
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0])


def cam_center(P):
    """C = -M^-1 p4 by Cramer's rule in fp64; None when det M = 0"""
    P = np.asarray(P, np.float64).reshape(3, 4)
    c = [[float(P[r, k]) for r in range(3)] for k in range(4)]
    det = det3(c[0], c[1], c[2])
    if det == 0.0 or not np.isfinite(det):
        return None
    return np.array([-(det3(c[3], c[1], c[2]) / det), -(det3(c[0], c[3], c[2]) / det), -(det3(c[0], c[1], c[3]) / det)], np.float64)


def vertex_normals(v, f):
    """the sum over each vertex's corners, in ascending 3 f + j, of its faces' (P1 - P0) x (P2 - P0) (fp64 from the float32 positions);
    faces with a repeated index take no part.  [nv, 3] float64, not normalised"""
    v = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    N = np.zeros((len(v), 3), np.float64)
    if len(f) == 0:
        return N
    ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    fn = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    corner = np.arange(3 * len(f))[np.repeat(ok, 3)]
    vert = f.reshape(-1)[corner]
    order = np.argsort(vert, kind="stable")                 # per vertex, corners ascending
    corner, vert = corner[order], vert[order]
    start = np.searchsorted(vert, np.arange(len(v)))
    rank = np.arange(len(vert)) - start[vert]
    for r in range(int(rank.max()) + 1 if len(rank) else 0):  # the r-th corner of every vertex: one sequential addition each
        m = rank == r
        N[vert[m]] += fn[corner[m] // 3]
    return N


def _edge(au, av, bu, bv, pu, pv):
    return (bu - au) * (pv - av) - (bv - av) * (pu - au)


def depth_buffer(v, f, P, W, H, return_items=False, big_box=4096):
    """one view's buffer, uint32 [H, W]: the largest float32 bit pattern of the inverse depth drawn at each pixel centre.  (Boxes of up
    to 8 x 8 pixels are walked for all faces at once, offset by offset, the others face by face: the same operations on every pixel.)"""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    buf = np.zeros(H * W, np.uint32)
    drawn = big = 0
    if len(f):
        q = project(P, v)
        with np.errstate(all="ignore"):
            uf, vf = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
            part = (q[:, 2] > 0) & np.isfinite(uf) & np.isfinite(vf)
            U, V, Wi = uf.astype(np.float64), vf.astype(np.float64), 1.0 / q[:, 2].astype(np.float64)
        f = f[part[f].all(axis=1)]
        u, vv, wi = U[f], V[f], Wi[f]                        # [m, 3]
        A = _edge(u[:, 0], vv[:, 0], u[:, 1], vv[:, 1], u[:, 2], vv[:, 2])
        x0, x1 = np.maximum(np.ceil(u.min(axis=1)), 0.0), np.minimum(np.floor(u.max(axis=1)), float(W - 1))
        y0, y1 = np.maximum(np.ceil(vv.min(axis=1)), 0.0), np.minimum(np.floor(vv.max(axis=1)), float(H - 1))
        keep = (A != 0.0) & (x0 <= x1) & (y0 <= y1)
        u, vv, wi, A = u[keep], vv[keep], wi[keep], A[keep]
        x0, x1, y0, y1 = (a[keep].astype(np.int64) for a in (x0, x1, y0, y1))
        bw, bh = x1 - x0 + 1, y1 - y0 + 1
        drawn, big = len(A), int((bw * bh > big_box).sum())
        s = np.where(A > 0.0, 1.0, -1.0)

        def draw(i, px, py):                                 # faces i (an index array or one index) at pixel centres (px, py)
            pu, pv = px.astype(np.float64), py.astype(np.float64)
            e0 = _edge(u[i, 1], vv[i, 1], u[i, 2], vv[i, 2], pu, pv)
            e1 = _edge(u[i, 2], vv[i, 2], u[i, 0], vv[i, 0], pu, pv)
            e2 = _edge(u[i, 0], vv[i, 0], u[i, 1], vv[i, 1], pu, pv)
            cov = (e0 * s[i] >= 0.0) & (e1 * s[i] >= 0.0) & (e2 * s[i] >= 0.0)
            with np.errstate(all="ignore"):
                w = ((e0 / A[i]) * wi[i, 0] + (e1 / A[i]) * wi[i, 1]) + (e2 / A[i]) * wi[i, 2]
                bits = w.astype(np.float32).view(np.uint32)
            np.maximum.at(buf, (py * W + px)[cov], bits[cov])

        small = (bw <= 8) & (bh <= 8)
        for dy in range(8):
            for dx in range(8):
                i = np.nonzero(small & (dx < bw) & (dy < bh))[0]
                if len(i):
                    draw(i, x0[i] + dx, y0[i] + dy)
        for i in np.nonzero(~small)[0]:
            ys, xs = np.mgrid[y0[i]:y1[i] + 1, x0[i]:x1[i] + 1]
            draw(i, xs.ravel(), ys.ravel())
    buf = buf.reshape(H, W)
    return (buf, drawn, big) if return_items else buf


def views_of(cams):
    """[(P, image, mask or None)] in scans.txt's order: every pair's view 0, then every pair's view 1"""
    return [(pair[k].P, pair[k].image, pair[k].mask) for k in range(2) for pair in cams]


def color(v, f, views, mode, min_cos, depth_eps, big_box=4096):
    """(rgb uint8 [nv, 3], best_view int32 [nv], stats dict) of DESIGN.md 9 f9; views: [(P, image BGR, mask or None)] in view order.
    mode "both": (rgb of mode 0, rgb of mode 1, best_view, stats) from one pass"""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    nv = len(v)
    N = vertex_normals(v, f)
    with np.errstate(all="ignore"):
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        has_n = length > 0.0
        n = N / np.where(has_n, length, 1.0)[:, None]
    p64 = v.astype(np.float64)
    best = np.full(nv, -1, np.int32)
    best_cos = np.zeros(nv)
    best_rgb = np.full((nv, 3), GREY, np.uint8)
    sw = np.zeros(nv)
    sc = np.zeros((nv, 3))
    n_vis = np.zeros(nv, np.int64)
    drawn = big = 0
    for k, (P, image, mask) in enumerate(views):
        img = np.asarray(image, np.uint8)
        H, W = img.shape[:2]
        buf, d, b = depth_buffer(v, f, P, W, H, True, big_box)
        drawn, big = drawn + d, big + b
        C = cam_center(P)
        q = project(P, v)
        x, y, inside = pixel_of(q, W, H)
        xi, yi = np.where(inside, x, 0), np.where(inside, y, 0)
        with np.errstate(all="ignore"):
            vis = has_n & (q[:, 2] > 0) & inside
            if mask is not None:
                vis &= np.asarray(mask, np.uint8)[yi, xi] == 255
            d0, d1, d2 = C[0] - p64[:, 0], C[1] - p64[:, 1], C[2] - p64[:, 2]
            cs = ((n[:, 0] * d0 + n[:, 1] * d1) + n[:, 2] * d2) / np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
            vis &= cs > min_cos
            wb = buf[yi, xi]
            vis &= (wb == 0) | (q[:, 2].astype(np.float64) <= 1.0 / wb.view(np.float32).astype(np.float64) + depth_eps)
        rgb_k = img[yi, xi][:, ::-1]                         # texture_color's colour there
        better = vis & ((best < 0) | (cs > best_cos))        # strict: a tie stays with the lower view
        best[better] = k
        best_cos[better] = cs[better]
        best_rgb[better] = rgb_k[better]
        w = np.where(vis & (cs > 0.0), cs, 0.0)              # a view let in by min_cos < 0 that faces away carries no weight
        sw += w
        sc += w[:, None] * rgb_k.astype(np.float64)
        n_vis += vis
    rgb = best_rgb.copy()
    m = (best >= 0) & (sw > 0.0)
    rgb[m] = (sc[m] / sw[m][:, None] + 0.5).astype(np.int64).astype(np.uint8)
    stats = dict(n_vertices=nv, coloured=int((best >= 0).sum()), no_normal=int((~has_n).sum()), visible_views=int(n_vis.sum()),
                 items_drawn=int(drawn), items_big_box=int(big))
    if mode == "both":
        return best_rgb, rgb, best, stats
    return (rgb if mode == 1 else best_rgb), best, stats


def look_at(eye, target, fx, cx, cy, up=(0.0, 1.0, 0.0)):
    """a 3x4 P = K [R | -R eye] of a camera at `eye` looking at `target` (z forward, x right, y down the image), fp64"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    K = np.array([[fx, 0.0, cx], [0.0, fx, cy], [0.0, 0.0, 1.0]])
    return K @ np.concatenate([R, (-R @ eye)[:, None]], axis=1)


def grid_plane(nx, ny, x0, y0, step, z):
    """an nx x ny lattice in the plane z, two faces per cell: (vertices float32, faces int32)"""
    xs, ys = np.meshgrid(x0 + step * np.arange(nx), y0 + step * np.arange(ny))
    v = np.stack([xs.ravel(), ys.ravel(), np.full(nx * ny, z)], axis=1).astype(np.float32)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + nx + 1], axis=1), np.stack([i, i + nx + 1, i + nx], axis=1)]).astype(np.int32)
    return v, f
