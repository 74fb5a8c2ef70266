"""An exact reference for the depth raster of the mesh colouring and the inputs that reach its edges.  It shares one
function with tests/meshcolor_restatement.py, project() (the float32 projection, pinned by hand and by texture_color); everything after
the float32 quotients u, v and the doubles w_i = 1 / (double)q2_i is decided in Python integers, from DESIGN's words and not from the
kernels' expressions: a pixel centre at integer coordinates inside the image is covered by a face when it lies in the closed triangle,
in either orientation; a face with a vertex of q2 <= 0, a quotient that is not finite or zero area draws nothing; the inverse depth is
the exact rational sum(lambda_i w_i) rounded ONCE to float32, to nearest even, straight from the rational; the buffer is the maximum of
those bit patterns.  No bounding box enters a decision: every pixel of the image is tested for every face.

Two tie rules, both derived from the arithmetic the kernels are allowed (fp64 basic operations), neither measured:
  coverage  a pixel-face decision is excused -- either answer passes -- when the least exact edge function E (times the sign of A)
            satisfies |E| <= 4 * 2^-53 * (|bu - au| |pv - av| + |bv - av| |pu - au|), the rounding an fp64 evaluation of
            (bu - au)(pv - av) - (bv - av)(pu - au) can carry (two differences, two products, one difference), UNLESS every one of those
            seven intermediate values is itself a double: then the fp64 evaluation is the exact E and nothing is excused.  (Without
            that clause every E = 0 would be excused; with it the dyadic and integer inputs, where every E is exact in fp64, excuse
            nothing.)  The area A is an edge function of the third vertex and is treated the same way: a face whose A is in doubt has
            all its decisions excused.
  value     a decision is excused when the exact w lies within 2^-48 relative of a float32 rounding midpoint: the fp64 tree of three
            quotients, three products and two sums of non-negative terms carries less than 2^-50.  A pixel passes when its bits lie
            between the maximum with every excused face rounded down (and every face whose coverage is excused left out) and the
            maximum with all of them rounded up (and let in).
Decisions are counted over the pixel centres of a face's exact box inside the image, the only ones a rasteriser decides.
The caps (conditions, not measurements): excused <= 1e-4 of a case's decisions and <= 1e-5 of all cases together; 0 on the cases marked
`exact` (dyadic and integer vertices)."""
import functools
from fractions import Fraction

import numpy as np

import meshcolor_restatement as mr                            # project() only

CAP_CASE, CAP_ALL = 1e-4, 1e-5
D = 2.0 ** -12                                                # the dyadic grid
EYE_P = np.hstack([np.eye(3), np.zeros((3, 1))])
F32_INF = 0x7F800000


def K_P(f, cx, cy):
    """K [I | 0] with focal length f (a power of two) and principal point (cx, cy)"""
    return np.array([[f, 0.0, cx, 0.0], [0.0, f, cy, 0.0], [0.0, 0.0, 1.0, 0.0]])


# ---- exact arithmetic ---------------------------------------------------------------------------------------------------------------------
def round_f32(N, Dn):
    """the positive rational N / Dn (Python integers) rounded to float32: (bits down, bits up, bits to nearest even, near) where down / up
    are the neighbours below and above (equal when N / Dn is a float32) and near says that N / Dn lies within 2^-48 relative of their
    midpoint.  Subnormals and the overflow to infinity included."""
    e = N.bit_length() - Dn.bit_length()                      # floor(log2(N / Dn)) is e or e - 1
    if (N if e >= 0 else N << -e) < (Dn << e if e >= 0 else Dn):
        e -= 1
    e = max(e, -126)                                          # below 2^-126 the spacing stays 2^-149
    sh = 23 - e
    num, den = (N << sh, Dn) if sh >= 0 else (N, Dn << -sh)
    m, r = divmod(num, den)                                   # N / Dn = (m + r / den) 2^(e - 23)

    def bits(k):
        return min(((e + 127) << 23) + k - (1 << 23), F32_INF)
    if r == 0:
        return bits(m), bits(m), bits(m), False
    up = 2 * r > den or (2 * r == den and (m & 1))
    near = (abs(2 * r - den) << 47) <= num                    # |r / den - 1/2| <= 2^-48 (num / den)
    return bits(m), bits(m + 1), bits(m + 1 if up else m), near


def is_double(n):
    """the integer n (times any power of two) has at most 53 significant bits"""
    n = abs(n)
    return n == 0 or (n >> ((n & -n).bit_length() - 1)).bit_length() <= 53


def edge_in_doubt(au, av, bu, bv, pu, pv):
    """E(a, b, p) over integers: (E, whether an fp64 evaluation of it may differ in sign or vanish where E does not)"""
    du, dv, qu, qv = bu - au, bv - av, pu - au, pv - av
    t0, t1 = du * qv, dv * qu
    E = t0 - t1
    if (abs(E) << 51) > abs(t0) + abs(t1):
        return E, False
    return E, not all(is_double(x) for x in (du, dv, qu, qv, t0, t1, E))


class Reference:
    """what reference() returns: lo / hi uint32 [H, W] (the buffer must lie between them), decisions, excused_cov, excused_val, and per face
    of the input: box (x0, x1, y0, y1 inside the image, or None when it draws nothing), clip (left, right, top, bottom: the box was cut
    there), covered (pixel centres certainly covered), on_edge (of those, with an edge function exactly 0)"""

    @property
    def excused(self):
        return self.excused_cov + self.excused_val

    def items(self, big_box):
        """(faces that draw, faces whose box inside the image holds more than big_box pixels): what the raster's counters must show"""
        boxes = [b for b in self.box if b is not None]
        return len(boxes), sum((b[1] - b[0] + 1) * (b[3] - b[2] + 1) > big_box for b in boxes)

    def mismatches(self, buf):
        buf = np.asarray(buf, np.uint32)
        return int(((buf < self.lo) | (buf > self.hi)).sum())


def reference(v, f, P, W, H):
    v = np.asarray(v, np.float32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    q = mr.project(P, v)
    with np.errstate(all="ignore"):
        uf, vf = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]        # float32 quotients
        wi = 1.0 / q[:, 2].astype(np.float64)
    takes_part = (q[:, 2] > 0) & np.isfinite(uf) & np.isfinite(vf)
    R = Reference()
    lo, hi = [0] * (W * H), [0] * (W * H)
    R.decisions = R.excused_cov = R.excused_val = 0
    R.box, R.clip, R.covered, R.on_edge = [], [], [], []
    for tri in f:
        R.box.append(None)
        R.clip.append((False,) * 4)
        R.covered.append(0)
        R.on_edge.append(0)
        if not takes_part[tri].all():
            continue
        fu = [Fraction(float(uf[i])) for i in tri]
        fv = [Fraction(float(vf[i])) for i in tri]
        fw = [Fraction(float(wi[i])) for i in tri]
        S = max(x.denominator for x in fu + fv)              # a power of two: u, v in units of 1 / S
        u, vv = [int(x * S) for x in fu], [int(x * S) for x in fv]
        Sw = max(x.denominator for x in fw)
        w = [int(x * Sw) for x in fw]
        A, A_doubt = edge_in_doubt(u[0], vv[0], u[1], vv[1], u[2], vv[2])
        if A == 0 and not A_doubt:
            continue
        bx0, bx1, by0, by1 = -((-min(u)) // S), max(u) // S, -((-min(vv)) // S), max(vv) // S   # ceil(min), floor(max)
        x0, x1, y0, y1 = max(bx0, 0), min(bx1, W - 1), max(by0, 0), min(by1, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        R.box[-1] = (x0, x1, y0, y1)
        R.clip[-1] = (bx0 < 0, bx1 > W - 1, by0 < 0, by1 > H - 1)
        n_box = (x1 - x0 + 1) * (y1 - y0 + 1)
        R.decisions += n_box
        if A == 0:                                            # (no area in exact arithmetic, but fp64 may see some: anything goes in its box)
            R.excused_cov += n_box
            for y in range(y0, y1 + 1):
                for x in range(x0, x1 + 1):
                    hi[y * W + x] = F32_INF
            continue
        s = 1 if A > 0 else -1
        # s E(a, b, p) = c0 + cx px + cy py over every pixel of the image, for the edges (b, c), (c, a), (a, b)
        coef = []
        for a, b in ((1, 2), (2, 0), (0, 1)):
            du, dv = u[b] - u[a], vv[b] - vv[a]
            coef.append((s * (dv * u[a] - du * vv[a]), s * (-dv * S), s * (du * S)))
        big = max(abs(c0) + abs(cx) * W + abs(cy) * H for c0, cx, cy in coef)
        dt = np.int64 if big < (1 << 62) else object
        py, px = (a.ravel() for a in np.mgrid[0:H, 0:W])
        if dt is object:                                      # Python integers, whatever their size
            xs, ys = np.array([int(x) for x in px], object), np.array([int(y) for y in py], object)
        else:
            xs, ys = px.astype(np.int64), py.astype(np.int64)
        E = [c0 + cx * xs + cy * ys for c0, cx, cy in coef]
        least = np.minimum(np.minimum(E[0], E[1]), E[2])
        inside = (least >= 0).astype(bool)
        # the pixels whose least edge function may be in doubt: |E| 2^51 <= the largest the bound takes over the image
        tmax = 0
        for a, b in ((1, 2), (2, 0), (0, 1)):
            tmax = max(tmax, abs(u[b] - u[a]) * max(abs(vv[a]), abs((H - 1) * S - vv[a])) + abs(vv[b] - vv[a]) * max(abs(u[a]), abs((W - 1) * S - u[a])))
        limit = tmax >> 51
        cand = (np.abs(least) <= limit).astype(bool) if dt is np.int64 else np.array([abs(int(e)) <= limit for e in least], bool)
        in_box = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        doubt = np.zeros(W * H, bool)
        for i in np.nonzero(cand & in_box)[0] if not A_doubt else ():
            j = min(range(3), key=lambda k: int(E[k][i]))
            a, b = ((1, 2), (2, 0), (0, 1))[j]
            doubt[i] = edge_in_doubt(u[a], vv[a], u[b], vv[b], int(px[i]) * S, int(py[i]) * S)[1]
        if A_doubt:
            doubt = in_box.copy()
        assert not (inside & ~in_box).any()                   # the closed triangle lies in its box
        R.excused_cov += int(doubt.sum())
        R.covered[-1] = int((inside & ~doubt).sum())
        R.on_edge[-1] = int((inside & ~doubt & (least == 0).astype(bool)).sum())
        den = abs(A) * Sw
        for i in np.nonzero(inside | doubt)[0]:
            num = sum(int(E[k][i]) * w[k] for k in range(3))  # w = sum(E_k w_k) / A
            if doubt[i]:                                      # either covered or not, and if covered the value of a pixel on the edge
                num = max(num, 1)
                hi[i] = max(hi[i], round_f32(num, den)[1])
                continue
            down, up, nearest, near = round_f32(num, den)
            if near:
                R.excused_val += 1
                lo[i], hi[i] = max(lo[i], down), max(hi[i], up)
            else:
                lo[i], hi[i] = max(lo[i], nearest), max(hi[i], nearest)
    R.lo, R.hi = np.array(lo, np.uint32).reshape(H, W), np.array(hi, np.uint32).reshape(H, W)
    return R


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """name, vertices float32 [n, 3], faces int32 [m, 3], P, W, H; exact: every E is exact in fp64 (excused must be 0); expect: per face,
    by construction, the number of pixel centres it covers (None: not stated)"""

    def __init__(self, name, tris, P, W, H, exact, expect=None, faces=None):
        self.name, self.P, self.W, self.H, self.exact = name, np.asarray(P, np.float64), W, H, exact
        uvz = np.asarray(tris, np.float64).reshape(-1, 3)
        fx, cx, fy, cy = self.P[0, 0], self.P[0, 2], self.P[1, 1], self.P[1, 2]
        z = uvz[:, 2]
        self.v = np.stack([(uvz[:, 0] - cx) * z / fx, (uvz[:, 1] - cy) * z / fy, z], axis=1).astype(np.float32)
        self.f = np.arange(len(uvz), dtype=np.int32).reshape(-1, 3) if faces is None else np.asarray(faces, np.int32)
        self.uvz, self.expect = uvz, expect
        if exact:                                             # the quotients are the intended coordinates, to the bit
            q = mr.project(self.P, self.v)
            ok = q[:, 2] > 0
            assert np.array_equal((q[:, 0] / q[:, 2])[ok].astype(np.float64), uvz[ok, 0]) and np.array_equal((q[:, 1] / q[:, 2])[ok].astype(np.float64), uvz[ok, 1])


def snap(x):
    return np.round(np.asarray(x, np.float64) / D) * D


def dyadic_tris(rng, n, lo, hi, scales, clip_lo=-20.0, clip_hi=70.0):
    """n triangles (u, v, z) on the 2^-12 grid: centres in [lo, hi), extents from `scales`, kept in (clip_lo, clip_hi), depths 1, 2, 4, 8"""
    c = rng.uniform(lo, hi, (n, 1, 2))
    uv = c + rng.uniform(-1, 1, (n, 3, 2)) * rng.choice(scales, (n, 1, 1))
    uv = np.clip(snap(uv), clip_lo + D, clip_hi - D)
    z = rng.choice([1.0, 2.0, 4.0, 8.0], (n, 3, 1))
    return np.concatenate([uv, z], axis=2)


def case_dyadic_soup(camera="eye"):
    """150 triangles on the 2^-12 grid in (-20, 70), from below a pixel to the whole range (a triangle of 90 x 90 is 2.3 images)"""
    rng = np.random.default_rng(4101 if camera == "eye" else 4102)
    t = dyadic_tris(rng, 150, (-10.0, -10.0), (58.0, 46.0), [0.3, 0.7, 3.0, 12.0, 40.0, 90.0])
    return Case("dyadic_soup_" + camera, t, EYE_P if camera == "eye" else K_P(4.0, 24.0, 18.0), 48, 36, True)


def case_integer_soup():
    """a 9 x 7 lattice of integer vertices (faces share edges and vertices, every other face turned over) and 40 free integer triangles:
    edges and vertices pass through pixel centres"""
    rng = np.random.default_rng(4103)
    nx, ny = 9, 7
    gx, gy = np.meshgrid(-4 + 7 * np.arange(nx), -5 + 7 * np.arange(ny))
    uv = np.stack([gx.ravel() + rng.integers(-2, 3, nx * ny), gy.ravel() + rng.integers(-2, 3, nx * ny)], axis=1).astype(np.float64)
    uvz = np.concatenate([uv, rng.choice([1.0, 2.0, 4.0, 8.0], (nx * ny, 1))], axis=1)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + nx + 1], axis=1), np.stack([i, i + nx + 1, i + nx], axis=1)])
    f[::2] = f[::2, ::-1]                                     # both orientations
    free = np.concatenate([rng.integers(-6, 54, (40, 3, 1)), rng.integers(-6, 42, (40, 3, 1)), rng.choice([1.0, 2.0, 4.0, 8.0], (40, 3, 1))], axis=2)
    f = np.concatenate([f, len(uvz) + np.arange(120).reshape(-1, 3)])
    return Case("integer_soup", np.concatenate([uvz, free.reshape(-1, 3)]), K_P(2.0, 8.0, 4.0), 48, 36, True, faces=f)


def case_general_soup(camera="eye"):
    """150 random triangles of every size at random depths: nothing is exact, the tie rules are in force"""
    rng = np.random.default_rng(4104 if camera == "eye" else 4105)
    n = 150
    c = rng.uniform(-10, 58, (n, 1, 2)) * [1.0, 46.0 / 58.0] + rng.uniform(-1, 1, (n, 3, 2)) * rng.choice([0.4, 3.0, 30.0, 60.0], (n, 1, 1))
    z = rng.uniform(1.0, 9.0, (n, 3, 1))
    return Case("general_soup_" + camera, np.concatenate([c, z], axis=2), EYE_P if camera == "eye" else K_P(32.0, 20.5, 17.25), 48, 36, False)


def case_slivers():
    """slivers on the 2^-12 grid that hold no pixel centre, exactly one, or exactly the row of centres one of their edges runs through"""
    t, n = [], []
    dirs = [(1, 0), (0, 1), (1, 1), (7, 3), (-2, 5), (12, 5), (-3, -1)]
    centres = [(0, 0), (47, 35), (47, 0), (0, 35), (20, 11), (33, 29), (8, 30)]
    for k, ((cx, cy), (p, q)) in enumerate(zip(centres, dirs)):
        z = [1.0, 2.0, 4.0, 8.0][k % 4]
        al = 15.0 / 16.0                                      # short of the next centre on the axis, c +- (p, q)
        tri = [(cx - al * p, cy - al * q, z), (cx + al * p - D * q, cy + al * q + D * p, z), (cx + al * p + D * q, cy + al * q - D * p, 2 * z)]
        t.append(tri if k % 2 else tri[::-1])
        n.append(1)
        # the same axis 2^-8 (-q, p) to the side, 4.5 (p, q) long either way: passes every centre of the axis, holds none
        ox, oy, al = -q / 256.0, p / 256.0, 4.5
        t.append([(cx + ox - al * p, cy + oy - al * q, z), (cx + ox + al * p - D * q, cy + oy + al * q + D * p, z), (cx + ox + al * p + D * q, cy + oy + al * q - D * p, z)])
        n.append(0)
    for x0, x1, y, side, z in ((3, 44, 7, 1, 1.0), (0, 47, 0, 1, 2.0), (0, 47, 35, -1, 4.0), (-5, 60, 20, -1, 8.0), (10, 11, 13, 1, 1.0)):
        t.append([(x0, y, z), (x1, y, z), ((x0 + x1) / 2.0, y + side * D, z)][::side])       # an edge along a row of centres
        n.append(min(x1, 47) - max(x0, 0) + 1)
    for x0, y0, k, z in ((2, 3, 30, 1.0), (-4, -4, 50, 2.0), (40, 2, 5, 4.0)):            # an edge along a diagonal of centres
        t.append([(x0, y0, z), (x0 + k, y0 + k, z), (x0 + k, y0 + k - D, 2 * z)])
        n.append(sum(0 <= x0 + j < 48 and 0 <= y0 + j < 36 for j in range(k + 1)))
    for x, y0, y1, z in ((0, 2, 30, 1.0), (47, -3, 40, 2.0), (25, 5, 6, 8.0)):            # and along a column
        t.append([(x, y0, z), (x, y1, z), (x - D, (y0 + y1) / 2.0, z)])
        n.append(min(y1, 35) - max(y0, 0) + 1)
    return Case("slivers", t, EYE_P, 48, 36, True, expect=n)


def case_tiny_and_zero_area():
    """areas of 2^-25 pixel and needles whose area is tiny next to their extent; three distinct collinear vertices and repeated ones (A = 0)"""
    t, n = [], []
    for x, y, z in ((0, 0, 1.0), (47, 35, 2.0), (13, 7, 4.0), (30, 20, 8.0)):
        t.append([(x, y, z), (x + D, y, z), (x, y + D, z)])                                # a vertex on the centre: that pixel
        n.append(1)
        t.append([(x, y, z), (x, y - D, z), (x - D, y, 2 * z)])                             # turned over
        n.append(1)
        t.append([(x + D, y + D, z), (x + 2 * D, y + D, z), (x + D, y + 2 * D, z)])        # beside it: none
        n.append(0)
    t.append([(0, 0, 1.0), (40, 30, 2.0), (40, 30 + D, 4.0)])                              # a needle: the centres (4 k, 3 k) of its edge
    n.append(11)
    t.append([(44, 2, 1.0), (4, 32, 1.0), (4 + D, 32, 1.0)])                               # ... (44 - 4 k, 2 + 3 k)
    n.append(11)
    t.append([(1, 1 + D, 1.0), (46, 1 + 2 * D, 1.0), (46, 1 + 3 * D, 1.0)])                # a needle between two rows: none
    n.append(0)
    for tri in ([(2, 3, 1.0), (10, 7, 2.0), (18, 11, 4.0)], [(5, 5, 1.0), (5, 20, 1.0), (5, 9, 8.0)], [(1.5, 2.25, 1.0), (3.5, 4.25, 1.0), (7.5, 8.25, 2.0)],
                [(0, 10, 1.0), (47, 10, 1.0), (20, 10, 1.0)], [(-3, 40, 2.0), (40, -3, 2.0), (20, 17, 1.0)], [(9, 9, 1.0), (9, 9, 1.0), (30, 12, 1.0)],
                [(6, 6, 1.0), (6, 6, 2.0), (6, 6, 4.0)], [(0.25, 0.5, 1.0), (0.25 + D, 0.5 + 3 * D, 1.0), (0.25 + 2 * D, 0.5 + 6 * D, 1.0)]):
        t.append(tri)                                         # collinear: nothing
        n.append(0)
    return Case("tiny_and_zero_area", t, K_P(2.0, 8.0, 4.0), 48, 36, True, expect=n)


def corner_tri(a, b, sx, sy, z=1.0, ex=3.5, ey=2.5):
    """the right triangle with its corner at (a, b), legs ex along sx and ey along sy: with sx = sy = 1 its box starts at (a, b), with
    -1 it ends there"""
    t = [(a, b, z), (a + sx * ex, b, z), (a, b + sy * ey, 2 * z)]
    return t if sx * sy > 0 else t[::-1]


def covered_by_corner_tri(a, b, sx, sy, W, H, ex=3.5, ey=2.5):
    """how many pixel centres of the image corner_tri holds, from its definition: sx (x - a) >= 0, sy (y - b) >= 0, and
    sx (x - a) / ex + sy (y - b) / ey <= 1, in exact rationals"""
    xr, yr = range(max(0, int(a - ex) - 2), min(W, int(a + ex) + 3)), range(max(0, int(b - ey) - 2), min(H, int(b + ey) + 3))
    a, b, ex, ey = Fraction(a), Fraction(b), Fraction(ex), Fraction(ey)
    return sum(1 for y in yr for x in xr if sx * (x - a) >= 0 and sy * (y - b) >= 0 and sx * (x - a) / ex + sy * (y - b) / ey <= 1)


def case_box():
    """the box's ends: minima and maxima exactly on an integer and 2^-12 either side of it, on the last column and row and 2^-12 past
    them, at -2^-12 and at -0.0, boxes cut at every border and corner, and boxes 2^-12 outside the image"""
    W, H = 48, 36
    t, n = [], []

    def add(a, b, sx, sy, **kw):
        t.append(corner_tri(a, b, sx, sy, **kw))
        n.append(covered_by_corner_tri(a, b, sx, sy, W, H, **{k: kw[k] for k in kw if k != "z"}))
    for da in (0.0, -D, D):
        for db in (0.0, -D, D):
            add(10 + da, 8 + db, 1, 1)                        # minima at 10 and 8, and beside them
            add(30 + da, 20 + db, -1, -1, z=2.0)              # maxima at 30 and 20
    for a in (47.0, 47.0 + D, 47.0 - D):
        add(a, 12.0, -1, 1)                                   # the maximum of u on the last column, past it, short of it
        add(a, 15.0, 1, 1)                                    # ... and the minimum there
    for b in (35.0, 35.0 + D, 35.0 - D):
        add(20.0, b, 1, -1)
        add(26.0, b, 1, 1)
    for a in (-D, 0.0, D):
        add(a, 25.0, 1, 1)                                    # the minimum of u at -2^-12, 0, 2^-12
        add(a, 29.0, -1, 1)                                   # the maximum there: column 0 or nothing
        add(36.0, a, 1, 1)
        add(41.0, a, 1, -1)
    for a, b, sx, sy in ((-2.0, -1.0, 1, 1), (49.0, -1.0, -1, 1), (-2.0, 36.0, 1, -1), (49.0, 36.0, -1, -1)):
        add(a, b, sx, sy, ex=9.0, ey=7.0)                     # cut at each corner
    for a, b, sx, sy in ((-3.0, 14.0, 1, 1), (50.0, 14.0, -1, 1), (14.0, -3.0, 1, 1), (14.0, 38.0, 1, -1)):
        add(a, b, sx, sy, ex=8.0, ey=6.0)                     # cut at each border
    t.append([(-30.0, -30.0, 4.0), (200.0, -30.0, 4.0), (-30.0, 200.0, 4.0)])               # cut at all four
    n.append(W * H)
    for tri in ([(-4.0, 5.0, 1.0), (-D, 5.0, 1.0), (-D, 9.0, 1.0)], [(47.0 + D, 5.0, 1.0), (52.0, 5.0, 1.0), (47.0 + D, 9.0, 1.0)],
                [(5.0, -4.0, 1.0), (5.0, -D, 1.0), (9.0, -D, 1.0)], [(5.0, 35.0 + D, 1.0), (5.0, 40.0, 1.0), (9.0, 35.0 + D, 1.0)]):
        t.append(tri)                                         # outside the image by 2^-12
        n.append(0)
    c = Case("box", t, EYE_P, W, H, True, expect=n)
    # -0.0: x = -2^-149 at depth 8 gives the float32 quotient -0.0 (and a rational 0); its triangle starts on column 0
    k = len(c.v)
    c.v = np.concatenate([c.v, np.float32([[-2.0 ** -149, 22.0 * 8.0, 8.0], [3.5 * 8.0, 22.0 * 8.0, 8.0], [-2.0 ** -149, 24.5 * 8.0, 8.0]])])
    c.f = np.concatenate([c.f, np.int32([[k, k + 1, k + 2]])])
    c.expect = n + [covered_by_corner_tri(0.0, 22.0, 1, 1, W, H)]
    c.minus_zero_vertex = k
    return c


def case_small_image(W, H):
    """a dyadic soup and integer triangles over an image of one row, one column, one pixel, or 257 x 3 (a row longer than a block)"""
    rng = np.random.default_rng(4200 + W + 1000 * H)
    m = float(max(W, H))
    t = dyadic_tris(rng, 40, (-3.0, -3.0), (W + 3.0, H + 3.0), [0.4, 2.0, m, 2.0 * m], clip_lo=-2.0 * m, clip_hi=3.0 * m)
    ti = np.concatenate([rng.integers(-2, W + 3, (20, 3, 1)), rng.integers(-2, H + 3, (20, 3, 1)), rng.choice([1.0, 2.0, 4.0, 8.0], (20, 3, 1))], axis=2)
    full = [[(-8.0, -8.0, 8.0), (4.0 * m + 32.0, -8.0, 8.0), (-8.0, 4.0 * m + 32.0, 8.0)]]              # the whole image, behind the others
    return Case("image_%dx%d" % (W, H), np.concatenate([t, ti, full]), EYE_P, W, H, True)


TIER_BIG_BOX = 12


def case_tier_switch():
    """boxes of exactly 12 and exactly 13 pixels, some only after the cut at the image: with meshcolor_big_box = 12 the first draw in the
    thread tier, the second in the block tier.  expect_big: per face, by hand"""
    t = [[(10, 10, 1.0), (12, 10, 1.0), (10, 13, 2.0)],       # 3 x 4
         [(20, 10, 1.0), (23, 10, 1.0), (20, 12, 2.0)],       # 4 x 3
         [(5, 20, 1.0), (16, 20, 1.0), (10, 20.5, 1.0)],      # 12 x 1
         [(30, 2, 1.0), (30.5, 8, 1.0), (30, 13, 2.0)],       # 1 x 12
         [(40, 2, 1.0), (41, 2, 1.0), (40, 7, 1.0)],          # 2 x 6
         [(36, 33, 2.0), (70, 33, 2.0), (36, 33.5, 2.0)],     # 35 x 1 cut to 12 x 1 by the right border
         [(2, 30, 4.0), (2.5, 30, 4.0), (2, 60, 4.0)],        # 1 x 31 cut to 1 x 6
         [(5, 22, 1.0), (17, 22, 1.0), (10, 22.5, 1.0)],      # 13 x 1
         [(33, 2, 1.0), (33.5, 8, 1.0), (33, 14, 2.0)],       # 1 x 13
         [(35, 34, 2.0), (70, 34, 2.0), (35, 34.5, 2.0)],     # 36 x 1 cut to 13 x 1
         [(20, 24, 1.0), (26, 24, 1.0), (20, 25, 1.0)],       # 7 x 2
         [(-30, -30, 8.0), (200, -30, 8.0), (-30, 200, 8.0)],  # the whole image
         [(44, 20, 1.0), (44 + D, 20, 1.0), (44, 20 + D, 1.0)]]  # one pixel
    c = Case("tier_switch", t, EYE_P, 48, 36, True)
    c.expect_big = [False] * 7 + [True] * 5 + [False]
    return c


def case_denormal():
    """u, v in {0, 1} at depth 2^127 on a 2 x 2 image: the inverse depth 2^-127 is subnormal in float32, 0x00400000 at three pixels"""
    z = 2.0 ** 127
    return Case("denormal", [[(0, 0, z), (1, 0, z), (0, 1, z)]], EYE_P, 2, 2, True, expect=[3])


def case_large():
    """depth 2^-120 (w = 2^120) and quotients up to float32's largest finite value: rows 6 .. 35 are inside triangles whose vertices lie
    at +-2^127 and +-FLT_MAX, their lower edge on v = 5.5; a quotient that overflows is skipped"""
    big, top = 2.0 ** 127, float(np.finfo(np.float32).max)
    t = [[(-big, 5.5, 1.0), (big, 5.5, 1.0), (0.0, big, 1.0)],
         [(top, 5.5, 0.5), (-top, 5.5, 0.5), (0.0, top, 0.5)],
         [(3, 2, 2.0 ** -120), (9, 2, 2.0 ** -120), (3, 5, 2.0 ** -120)],
         [(20, 1, 2.0 ** -120), (30, 1, 1.0), (20, 5, 1.0)],
         [(40, 1, 2.0 ** -100), (46, 1, 2.0 ** -110), (40, 5, 2.0 ** -120)]]
    c = Case("large", t, EYE_P, 48, 36, True)
    k = len(c.v)                                              # 3e38 / 0.5 overflows float32: the face is skipped
    c.v = np.concatenate([c.v, np.float32([[3e38, 1.0, 0.5], [1.0, 3e38, 0.5], [5.0, 5.0, 1.0]])])
    c.f = np.concatenate([c.f, np.int32([[k, k + 1, k + 2]])])
    return c


BUILDERS = {
    "dyadic_soup_eye": lambda: case_dyadic_soup("eye"),
    "dyadic_soup_K": lambda: case_dyadic_soup("K"),
    "integer_soup": case_integer_soup,
    "general_soup_eye": lambda: case_general_soup("eye"),
    "general_soup_K": lambda: case_general_soup("K"),
    "slivers": case_slivers,
    "tiny_and_zero_area": case_tiny_and_zero_area,
    "box": case_box,
    "image_1x1": lambda: case_small_image(1, 1),
    "image_1x40": lambda: case_small_image(1, 40),
    "image_40x1": lambda: case_small_image(40, 1),
    "image_257x3": lambda: case_small_image(257, 3),
    "tier_switch": case_tier_switch,
    "denormal": case_denormal,
    "large": case_large,
}
CASES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c.name == name
    return c


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the exact reference of a case, computed once"""
    c = case(name)
    return reference(c.v, c.f, c.P, c.W, c.H)


def hold(name, buf, label):
    """the raster check of one case: prints the counts, asserts the buffer and the case's cap"""
    c, R = case(name), case_reference(name)
    bad = R.mismatches(buf)
    print("%s %s: %d faces, %d decisions, %d on an edge exactly, excused %d (coverage) + %d (value); pixels outside the reference: %d of %d"
          % (label, name, len(c.f), R.decisions, sum(R.on_edge), R.excused_cov, R.excused_val, bad, c.W * c.H))
    assert bad == 0
    assert R.excused <= CAP_CASE * R.decisions
    if c.exact:
        assert R.excused == 0
    return R


# ---- visibility and colour: scenes with answers known beforehand ----------------------------------------------------------------------------
# Every scene is planar with vertex normals exactly (0, 0, -1) (the faces' cross products have no x or y part), seen by cameras
# K [I | -C] whose centre Cramer's rule returns exactly (small integers and powers of two).  A scene: vertices, faces, a list of pairs
# [(P, image, mask), (P, image, mask)], min_cos, depth_eps, the probe's vertex index, and the answer (best_view, rgb) -- (-1, grey) when
# no view may see it.
GREY = (127, 127, 127)


def solid(W, H, rgb):
    img = np.empty((H, W, 3), np.uint8)
    img[:] = rgb[::-1]                                        # BGR
    return img


def cam(f, cx, cy, C=(0.0, 0.0, 0.0)):
    """K [I | -C]"""
    K = np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
    return K @ np.hstack([np.eye(3), -np.asarray(C, np.float64).reshape(3, 1)])


def probe_tri(p):
    """a triangle in the plane z = p_z with the probe p as its first vertex and the normal (0, 0, -1)"""
    p = np.asarray(p, np.float64)
    return [p, p + [0.0, 1.0, 0.0], p + [1.0, 0.0, 0.0]]


class Scene:
    def __init__(self, name, v, f, pairs, min_cos, depth_eps, probe, best, rgb, rgb_blend=None):
        self.name, self.v, self.f, self.pairs = name, np.asarray(v, np.float32), np.asarray(f, np.int32), pairs
        self.min_cos, self.depth_eps, self.probe, self.best, self.rgb = min_cos, depth_eps, probe, best, tuple(rgb)
        self.rgb_blend = rgb_blend                            # mode 1: real-valued channels to within 1/2, or None: the same colour as mode 0


def blind(P, W, H):
    """a view that sees nothing: mask 0"""
    return (P, solid(W, H, (9, 9, 9)), np.zeros((H, W), np.uint8))


def scenes_depth():
    """a plane at depth 8 over the whole 16 x 12 image (the buffer holds 1/8); the probe behind it on the ray of pixel (8, 6), depth_eps
    0.5: visible at q2 = 8.5, hidden at the next float32"""
    W, H, P = 16, 12, cam(16.0, 8.0, 6.0)
    plane = [[-8.0, -8.0, 8.0], [8.0, -8.0, 8.0], [8.0, 8.0, 8.0], [-8.0, 8.0, 8.0]]     # u = 8 -+ 16, v = 6 -+ 16
    out = []
    for name, z, best in (("at_8.5", np.float32(8.5), 0), ("next_above_8.5", np.nextafter(np.float32(8.5), np.float32(9)), -1),
                          ("next_below_8.5", np.nextafter(np.float32(8.5), np.float32(8)), 0)):
        v = plane + probe_tri([0.0, 0.0, float(z)])
        f = [[0, 2, 1], [0, 3, 2], [4, 5, 6]]
        pairs = [[(P, solid(W, H, (200, 100, 50)), None), blind(P, W, H)]]
        out.append(Scene("depth_" + name, v, f, pairs, 0.2, 0.5, 4, best, (200, 100, 50) if best == 0 else GREY))
    return out


def scenes_undrawn():
    """an edge-on face (a line in the image: A = 0, nothing drawn, the buffer stays 0) seen along +x: its vertices are visible whatever
    their depth, with cos = 0 > min_cos = -0.5; weight 0 in the blend, so the best view's colour in both modes"""
    W, H = 16, 12
    K = np.array([[16.0, 0.0, 8.0], [0.0, 16.0, 6.0], [0.0, 0.0, 1.0]])
    R = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])                       # camera z = world x, camera x = world y
    P = K @ np.hstack([R, np.zeros((3, 1))])
    v = [[4.0, -1.0, 0.0], [4.0, 1.0, 0.0], [8.0, 0.0, 0.0]]                                # pixels (4, 6), (12, 6), (8, 6); normal (0, 0, -1)
    pairs = [[(P, solid(W, H, (10, 220, 30)), None), (P, solid(W, H, (250, 0, 0)), None)]]
    return [Scene("undrawn_depth_%d" % (4 if k < 2 else 8), v, [[0, 1, 2]], pairs, -0.5, 0.0, k, 0, (10, 220, 30)) for k in (0, 2)]


def scenes_angle():
    """C - p = (3, 0, -4) with the normal (0, 0, -1): cos is the double 0.8.  min_cos = 0.8 shuts the view out (the comparison is strict),
    the double below 0.8 lets it in"""
    W, H, P = 32, 24, cam(16.0, 16.0, 12.0)
    out = []
    for name, mc, best in (("at_0.8", 0.8, -1), ("below_0.8", float(np.nextafter(0.8, 0.0)), 0), ("above_0.8", float(np.nextafter(0.8, 1.0)), -1)):
        pairs = [[(P, solid(W, H, (1, 2, 250)), None), blind(P, W, H)]]
        out.append(Scene("angle_" + name, probe_tri([-3.0, 0.0, 4.0]), [[0, 1, 2]], pairs, mc, 0.5, 0, best, (1, 2, 250) if best == 0 else GREY))
    return out


def scenes_mask():
    """the probe on pixel (8, 6): mask 255 there lets the view in, 254 and 0 do not (the rest of the mask is the opposite)"""
    W, H, P = 16, 12, cam(16.0, 8.0, 6.0)
    out = []
    for val, best in ((255, 0), (254, -1), (0, -1)):
        m = np.full((H, W), 0 if val == 255 else 255, np.uint8)
        m[6, 8] = val
        pairs = [[(P, solid(W, H, (70, 80, 90)), m), blind(P, W, H)]]
        out.append(Scene("mask_%d" % val, probe_tri([0.0, 0.0, 4.0]), [[0, 1, 2]], pairs, 0.2, 0.5, 0, best, (70, 80, 90) if best == 0 else GREY))
    return out


def scenes_view_order():
    """three pairs; two mirror-image cameras at (+-3, 0, 0) see the probe (0, 0, 4) at bit-equal cos 0.8, as pair 2's view 0 (v = 2) and
    pair 0's view 1 (v = 3); the other four see nothing.  The tie goes to the lower v = k n_pairs + i, whichever camera sits there"""
    W, H = 32, 24
    left, right = cam(16.0, 16.0, 12.0, (-3.0, 0.0, 0.0)), cam(16.0, 16.0, 12.0, (3.0, 0.0, 0.0))
    out = []
    for name, first, second in (("left_first", left, right), ("right_first", right, left)):
        c0, c1 = ((11, 22, 33), (211, 222, 233)) if first is left else ((211, 222, 233), (11, 22, 33))
        P0 = cam(16.0, 16.0, 12.0)
        pairs = [[blind(P0, W, H), (second, solid(W, H, c1), None)],       # pair 0: v = 0, 3
                 [blind(P0, W, H), blind(P0, W, H)],                       # pair 1: v = 1, 4
                 [(first, solid(W, H, c0), None), blind(P0, W, H)]]        # pair 2: v = 2, 5
        blend = tuple((a + b) / 2.0 for a, b in zip(c0, c1))
        out.append(Scene("view_order_" + name, probe_tri([0.0, 0.0, 4.0]), [[0, 1, 2]], pairs, 0.2, 0.5, 0, 2, c0, blend))
    return out


MANY_PAIRS = 40
MANY_FORCED = (0, 39, 40, 63, 64, 79)


def scenes_many_views():
    """40 pairs of 4 x 4 images, 80 views: 79 cameras at (3, 0, 0) see the probe (0, 0, 4) at cos 0.8 and the forced one, at the origin,
    at cos 1; view v's image is the solid colour (v, 255 - v, 7)"""
    W, H = 4, 4
    side, front = cam(1.0, 2.0, 2.0, (3.0, 0.0, 0.0)), cam(1.0, 2.0, 2.0)
    out = []
    for forced in MANY_FORCED:
        col = lambda v: (v, 255 - v, 7)
        view = lambda v: (front if v == forced else side, solid(W, H, col(v)), None)
        pairs = [[view(i), view(MANY_PAIRS + i)] for i in range(MANY_PAIRS)]
        wsum = 1.0 + 0.8 * 79
        blend = tuple((col(forced)[c] + 0.8 * sum(col(v)[c] for v in range(80) if v != forced)) / wsum for c in range(3))
        out.append(Scene("many_views_%d" % forced, probe_tri([0.0, 0.0, 4.0]), [[0, 1, 2]], pairs, 0.2, 0.5, 0, forced, col(forced), blend))
    return out


@functools.lru_cache(maxsize=None)
def scenes():
    out = scenes_depth() + scenes_undrawn() + scenes_angle() + scenes_mask() + scenes_view_order() + scenes_many_views()
    return {s.name: s for s in out}


SCENES = ["depth_at_8.5", "depth_next_above_8.5", "depth_next_below_8.5", "undrawn_depth_4", "undrawn_depth_8", "angle_at_0.8", "angle_below_0.8",
          "angle_above_0.8", "mask_255", "mask_254", "mask_0", "view_order_left_first", "view_order_right_first"] + ["many_views_%d" % v for v in MANY_FORCED]


def hold_scene(s, mode, rgb, best):
    """the probe's answer in one mode"""
    got, b = tuple(int(x) for x in rgb[s.probe]), int(best[s.probe])
    print("%s mode %d: best view %d (want %d), colour %s" % (s.name, mode, b, s.best, got))
    assert b == s.best
    if mode == 1 and s.rgb_blend is not None:
        assert all(abs(g - r) <= 0.5 + 1e-9 for g, r in zip(got, s.rgb_blend))
    else:
        assert got == s.rgb
