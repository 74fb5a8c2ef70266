"""Inputs for the constraint-stage tests (tests/test_constraints_cpu.py, tests/test_gpu_constraint_chains.py): built by
construction, numpy only.  Whether a construction reaches what it is for is asserted in test_constraints_cpu.py from the class
maps and row statistics of tests/constraints_restatement.py -- never from what a kernel returns.

Uniqueness chains.  A pixel x of value v looks at q[bL .. bL+2] with bL = int(v + 0.5) + x - 1 and, failing a direct match, at
t = bL + 1 only.  Values in arithmetic progression along the row (step +2: t advances by 3; step -3 on negative values: t
retreats by 2) with q[t(x)] = -p[x-1] and every other q NOMATCH give pixels that have no direct match (|q + p[x]| = |step|),
are not rescued by p[x+1] (|p[x+1] - p[x-1]| = 2 |step|) and live exactly as long as p[x-1] does: class 3."""
import numpy as np

NOMATCH = -10000
E40 = 2.0 ** -40


class Fx(dict):
    __getattr__ = dict.__getitem__


def _blank(H, W, dtype):
    return np.full((H, W), NOMATCH, dtype), np.full((H, W), NOMATCH, dtype)


def _target(v, x, XL1):
    return max(int(v + 0.5) + x - 1, XL1) + 1


def put_chain(p, q, y, x0, L, oth, step=2, head="direct", frac=0.0):
    """Pixels x0 .. x0 + L in progression; x0 is the head: 'direct' (kept by a direct match), 'dead' (nothing keeps it) or
    'prev' (kept by p[x0 - 1], which is written too: x0 is meant to be XL).  The L pixels after it are class 3 or 4."""
    XL1, XR1 = oth[2], oth[3]
    base = 0 if step > 0 else step
    val = lambda k: base + step * k + frac
    lo = -1 if head == "prev" else 0
    for k in range(lo, L + 1):
        p[y, x0 + k] = val(k)
    for k in range(0, L + 1):
        x = x0 + k
        t = _target(val(k), x, XL1)
        assert XL1 + 1 < t < XR1 - 1 and q[y, t] == NOMATCH and q[y, t - 1] == NOMATCH and q[y, t + 1] == NOMATCH, (y, x, t)
        if k > 0 or head == "prev":
            q[y, t] = -val(k - 1)
        elif head == "direct":
            q[y, t] = -val(0)


def put_by_next(p, q, y, x, oth, v=0, w=5):
    """A pixel kept by p[x+1] alone (class 2); p[x+1] = w is written (inside the margin it is a pixel of its own: it dies)."""
    p[y, x], p[y, x + 1] = v, w
    t = _target(v, x, oth[2])
    assert q[y, t] == NOMATCH
    q[y, t] = -w


def _margins(H, W, XL, XR, XL1=2, XR1=None):
    XR1 = W - 3 if XR1 is None else XR1
    return (0, H - 1, XL, XR, XR - XL + 1, H), (0, H - 1, XL1, XR1, XR1 - XL1 + 1, H)


RUN_LENGTHS = (1, 2, 63, 64, 65)
END_LANES = (62, 63, 0, 1)


def _long(dtype, step, frac):
    """Rows 0/1: a head 20 columns into chunk 0 and 135 class-3 pixels (two chunk boundaries), alive and with the head dead.
    Rows 2/3: a run from XL rescued by p[XL-1], and the same with p[XL-1] NOMATCH.  Row 4: class 2 at lanes 63 and at XR."""
    H, W, XL = 5, 900, 320 if step < 0 else 6
    XR = XL + 200
    own, oth = _margins(H, W, XL, XR)
    p, q = _blank(H, W, dtype)
    put_chain(p, q, 0, XL + 20, 135, oth, step, "direct", frac)
    put_chain(p, q, 1, XL + 20, 135, oth, step, "dead", frac)
    put_chain(p, q, 2, XL, 140, oth, step, "prev", frac)
    put_chain(p, q, 3, XL, 140, oth, step, "prev", frac)
    p[3, XL - 1] = NOMATCH
    for x in (XL + 63, XL + 127, XR):
        put_by_next(p, q, 4, x, oth, v=0 + frac, w=5 + frac)
    return Fx(p=p, q=q, own=own, oth=oth, chain=True)


def _lanes(dtype, step, frac, head):
    """One run per row: every length of RUN_LENGTHS ending at every lane of END_LANES of chunk 2 or 3."""
    H, W, XL = len(RUN_LENGTHS) * len(END_LANES), 1000, 330 if step < 0 else 5
    XR = XL + 64 * 3 + 30
    own, oth = _margins(H, W, XL, XR)
    p, q = _blank(H, W, dtype)
    y = 0
    for L in RUN_LENGTHS:
        for lane in END_LANES:
            end = XL + 64 * (3 if lane < 2 else 2) + lane
            put_chain(p, q, y, end - L, L, oth, step, head, frac)
            y += 1
    return Fx(p=p, q=q, own=own, oth=oth, chain=True)


WIDTH_ROWS = ((1, 1), (63, 3), (64, 4), (65, 5), (128, 3), (129, 5))


def _width(dtype, width, rows):
    """Margin of `width` columns and `rows` rows; row r: 0 a run over the whole margin kept by p[XL-1], 1 the same with
    p[XL-1] NOMATCH, 2 a class-2 pixel at XR; then again."""
    H, W, XL = rows, 3 * width + 40, 4
    XR = XL + width - 1
    own, oth = _margins(H, W, XL, XR)
    p, q = _blank(H, W, dtype)
    for y in range(rows):
        if y % 3 == 2:
            put_by_next(p, q, y, XR, oth)
        else:
            put_chain(p, q, y, XL, width - 1, oth, 2, "prev")
            if y % 3 == 1:
                p[y, XL - 1] = NOMATCH
    return Fx(p=p, q=q, own=own, oth=oth, chain=True)


FRACTIONS = (0.0, 0.5, -0.5, 0.25, -0.25, 0.75, -0.75)
NOISE_F64 = (0.0, 1.0, -1.0, 2.0, -2.0, 2 - E40, -(2 - E40), 2 + E40, -(2 + E40), 1.5, -1.5)


def _clamps(dtype, seed):
    """Random maps under an other-view margin much narrower than the own one, the margin rows reaching the buffer's last row:
    boundary_L clamped up to XL1, boundary_R clamped to XR1, empty candidate loops with q[boundary_L+1] read beyond XR1, from
    the next row and from beyond the buffer.  q is written where the pixels look, with what they look for or nearly so."""
    rng = np.random.default_rng(seed)
    H, W = 6, 96
    own, oth = (0, H - 1, 4, 91, 88, H), (0, H - 1, 30, 70, 41, H)
    flt = dtype == np.float64
    p = rng.integers(-5, 6, size=(H, W)).astype(dtype)
    far = (rng.random((H, W)) < 0.15) & (np.arange(W)[None, :] > 55)
    p[far] = rng.integers(8, 45, size=int(far.sum()))
    if flt:
        p += rng.choice(FRACTIONS, size=(H, W))
    p[rng.random((H, W)) < 0.25] = NOMATCH
    q = rng.integers(-5, 6, size=(H, W)).astype(dtype)
    q[rng.random((H, W)) < 0.5] = NOMATCH
    pf, qf = p.ravel(), q.ravel()
    noise = NOISE_F64 if flt else (0, 1, -1, 2, -2)
    for y in range(H):
        for x in range(own[2], own[3] + 1):
            v = p[y, x]
            if v == NOMATCH or rng.random() < 0.3:
                continue
            i = y * W + _target(v, x, oth[2]) + int(rng.integers(-1, 2)) * int(rng.random() < 0.4)
            src = pf[y * W + x + int(rng.integers(-1, 2))]
            if 0 <= i < H * W and src != NOMATCH:
                qf[i] = -src + noise[int(rng.integers(0, len(noise)))]
    return Fx(p=p, q=q, own=own, oth=oth, chain=False)


def _thresholds():
    """float64: isolated triples whose deciding sum is exactly 2 - 2^-40, 2 or 2 + 2^-40, on both signs, as the direct match,
    as the p[x+1] test and as the p[x-1] test."""
    H, W = 3, 200
    own, oth = _margins(H, W, 4, 190)
    p, q = _blank(H, W, np.float64)
    x = 8
    for role in range(3):
        for s in (2 - E40, 2.0, 2 + E40):
            for sign in (1.0, -1.0):
                v = 1.0
                p[role, x - 1], p[role, x], p[role, x + 1] = 9.0, v, -7.0
                t = _target(v, x, oth[2])
                q[role, t] = -(v, -7.0, 9.0)[role] + sign * s
                q[role, x + 8] = -9.0           # p[x-1] has a direct match of its own: it is alive when x looks at it
                x += 10
        x = 8
    return Fx(p=p, q=q, own=own, oth=oth, chain=False)


def _plus_nomatch(dtype):
    """q[boundary_L+1] within 2 of +10000 = -NOMATCH: the first test of :492 then holds against a p[x-1] that READS NOMATCH --
    a pixel that was never valid or one the loop has just killed -- and fails against a live one.  (A disparity of +10000
    is a column offset a 16384-wide pair can have.)  Groups x-1, x, x+1 with p[x] = 0, p[x+1] = 2 chained on p[x]:
    row 0 p[x-1] NOMATCH, row 1 p[x-1] valid and killed, row 2 p[x-1] alive, row 3 as row 1 at lanes 0 and 63."""
    H, W, XL = 4, 420, 6
    own, oth = _margins(H, W, XL, XL + 340)
    p, q = _blank(H, W, dtype)
    offs = (-2, -1, 0, 1, 2) if dtype == np.int16 else (-2.0, -(2 - 2.0 ** -30), -1.0, 0.0, 1.5, 2 - 2.0 ** -30, 2.0)   # 10000 + e is exact

    def group(y, x, prev, e):
        p[y, x], p[y, x + 1] = 0, 2
        q[y, x] = 10000 + e             # t(x) = x
        q[y, x + 3] = 0                 # t(x+1) = x + 3: -p[x]
        if prev != "invalid":
            p[y, x - 1] = 20            # looks at q[x+18 .. x+20]
            if prev == "alive":
                q[y, x + 19] = -20

    for y, prev in enumerate(("invalid", "killed", "alive")):
        for i, e in enumerate(offs):
            group(y, XL + 10 + 40 * i, prev, e)
    for i, e in enumerate(offs[1:4]):
        group(3, XL + 64 * (2 * i + 1), "killed", e)        # x at lane 0: the killed p[x-1] is lane 63 of the chunk before
    group(3, XL + 64 * 4 - 1, "killed", 0)                  # x at lane 63: the pixel chained on it is lane 0 of the next chunk
    return Fx(p=p, q=q, own=own, oth=oth, chain=True)


def uniqueness_fixtures():
    """name -> Fx(p, q, own, oth, chain).  int16 and float64 of every construction; the float64 ones carry fractions."""
    out = {}
    for nm, dt, fp, fn in (("s16", np.int16, 0.0, 0.0), ("f64", np.float64, 0.25, -0.3)):
        out["long_pos_" + nm] = _long(dt, 2, fp)
        out["long_neg_" + nm] = _long(dt, -3, fn)
        out["lanes_pos_" + nm] = _lanes(dt, 2, fp, "direct")
        out["lanes_neg_dead_" + nm] = _lanes(dt, -3, fn, "dead")
        for w, r in WIDTH_ROWS:
            out["width%d_rows%d_%s" % (w, r, nm)] = _width(dt, w, r)
        for seed in (1, 2, 3):
            out["clamps%d_%s" % (seed, nm)] = _clamps(dt, seed)
        out["plus_nomatch_" + nm] = _plus_nomatch(dt)
    out["thresholds_f64"] = _thresholds()
    return out


def uniq_intervals(p, own, oth):
    """raw = int(p + 0.5) + x - 1, boundary_L and boundary_R of every valid pixel of the own margin (else None)."""
    H, W = p.shape
    res = {}
    for y in range(own[0], own[1] + 1):
        for x in range(own[2], own[3] + 1):
            v = p[y, x].item()
            if v != NOMATCH:
                raw = int(v + 0.5) + x - 1
                bl = max(raw, oth[2])
                res[(y, x)] = (raw, bl, min(bl + 2, oth[3]))
    return res


# ---------------------------------------------------------------- OrderConstraint
ORDER_ONE_COMPONENT = (47, 48, 49, 50, 96, 97)


def order_narrow():
    """Fx(d, own, rows): rows[y] = dict(kind, and what the row is built to have: n, components, longest, spread or ends)."""
    rng = np.random.default_rng(11)
    W, XL = 400, 3
    rows, ds = [], []

    def row():
        ds.append(np.full(W, NOMATCH, np.int16))
        return ds[-1]

    for n in ORDER_ONE_COMPONENT:
        for gaps in (False, True):
            d = row()
            xs = XL + (np.sort(rng.choice(np.arange(2 * n), n, replace=False)) if gaps else np.arange(n))
            d[xs] = rng.integers(-6, 7, n)
            d[xs[0]] = xs[-1] - xs[0] + 8          # the ends cross every pixel between them: one component
            d[xs[-1]] = -(xs[-1] - xs[0] + 8)
            rows.append(dict(kind="one", n=n, components=1, longest=n))
    d = row(); d[XL:XL + 120] = 3
    rows.append(dict(kind="spread", n=120, spread=0, components=0))
    d = row(); d[XL:XL + 120] = rng.integers(0, 2, 120); d[XL] = 0; d[XL + 1] = 1
    rows.append(dict(kind="spread", n=120, spread=1, components=0))
    d = row(); xs = XL + np.arange(0, 60, 3); d[xs] = rng.integers(-30, 31, 20); d[xs[0]] = 30; d[xs[1]] = -30
    rows.append(dict(kind="wide_spread", n=20))
    # components ending at list positions 63, 64, 127, 128: a block's first pixel is lifted to the block's last column + 1
    d = row(); d[XL:XL + 150] = 0
    ends = (63, 64, 127, 128, 149)
    start = 0
    for e in ends:
        if e > start:
            d[XL + start] = e - start + 1
            d[XL + start + 2] = 2               # and a second, local crossing inside the block
        start = e + 1
    rows.append(dict(kind="ends", n=150, ends=list(ends), components=3, longest=64))
    H = len(ds)
    return Fx(d=np.stack(ds), own=(0, H - 1, XL, W - 4, W - 3 - XL, H), rows=rows)


ORDER_WIDE_WIDTHS = (10432, 10433, 10496, 16382)
ORDER_WIDE_KINDS = ("ordered", "tied_by_both_ends", "local_inversions", "every_second_random", "one_pixel", "local_inversions")


def order_wide(width, inversions=300):
    """Six margin rows of `width` columns in a map of width + 2, one kind each (p + x stays within int16)."""
    rng = np.random.default_rng(width)
    W, H = width + 2, len(ORDER_WIDE_KINDS)
    d = np.full((H, W), NOMATCH, np.int16)
    for y, kind in enumerate(ORDER_WIDE_KINDS):
        r = d[y, 1:W - 1]
        if kind == "ordered":
            r[:] = (np.arange(width) // 700) % 2      # 1 -> 0 makes two equal p + x: a tie, no crossing
        elif kind == "tied_by_both_ends":
            r[:] = rng.integers(0, 2, width)
            r[0], r[-1] = width + 3, -(width + 3)
        elif kind == "local_inversions":
            r[:] = 0
            r[rng.choice(np.arange(4, width - 8), inversions, replace=False)] = 3
        elif kind == "every_second_random":
            r[::2] = rng.integers(-8, 9, len(r[::2]))
        elif kind == "one_pixel":
            r[width // 3] = 5
    return Fx(d=d, own=(0, H - 1, 1, W - 2, width, H))


# ---------------------------------------------------------------- SetBoundary / uniqueness at the widest row
def wide_maps(seed, dtype=np.int16, W=16384, H=40):
    rng = np.random.default_rng(seed)
    own, oth = (1, H - 2, 1, W - 2, W - 2, H - 2), (1, H - 2, 3, W - 7, W - 9, H - 2)
    d = rng.integers(-4, 6, size=(H, W)).astype(np.int16)
    d[rng.random((H, W)) < 0.3] = NOMATCH
    mask = np.where(rng.random((H, W)) < 0.85, 255, rng.integers(0, 255, size=(H, W))).astype(np.uint8)
    for y, alone in ((9, True), (22, False)):     # all-255 mask rows holding one valid pixel: one carry through every chunk
        mask[y] = 255
        d[y] = NOMATCH
        d[y, 8000 + y] = 2
        if alone:                                 # nothing arrives from above or below either
            mask[y - 1] = 0
            mask[y + 1] = 0
    q = rng.integers(-4, 6, size=(H, W)).astype(np.int16)
    q[rng.random((H, W)) < 0.2] = NOMATCH
    ys, xs = np.nonzero(d != NOMATCH)
    sel = slice(None, None, 3)
    t = xs[sel] + d[ys[sel], xs[sel]]
    ok = (t >= 0) & (t < W)
    q[ys[sel][ok], t[ok]] = -d[ys[sel][ok], xs[sel][ok]] + rng.integers(-2, 3, int(ok.sum()))
    if dtype == np.float64:
        pf = np.where(d == NOMATCH, float(NOMATCH), d + rng.choice(FRACTIONS, size=d.shape))
        qf = np.where(q == NOMATCH, float(NOMATCH), q + rng.choice(FRACTIONS, size=q.shape))
        return Fx(p=pf, q=qf, mask=mask, own=own, oth=oth)
    return Fx(p=d, q=q, mask=mask, own=own, oth=oth)


# ---------------------------------------------------------------- SmoothConstraint / MedianFilter at the 256-column blocks
BLOCK_WIDTHS = (255, 256, 257, 513)
BLOCK_HEIGHTS = (1, 2, 5)
BLOCK_INSETS = (1, 4)
BLOCK_SHARES = (0.0, 0.3, 0.9)


def block_cases(width):
    """Every (height, inset, W, NOMATCH share) for a margin of `width` columns: the map tight round the margin (inset pixels
    on every side), and with the right border moved so that 2 XR lies below W, at W - 1, W, W + 1 and above it."""
    seed = 0
    for h in BLOCK_HEIGHTS:
        for inset in BLOCK_INSETS:
            XL, YL = inset, inset
            XR, YR = XL + width - 1, YL + h - 1
            for W in (XR + 1 + inset, 2 * XR + 6, 2 * XR + 1, 2 * XR, 2 * XR - 1, 2 * XR - 8):
                for share in BLOCK_SHARES:
                    seed += 1
                    rng = np.random.default_rng(1000 * width + seed)
                    H = YR + 1 + inset
                    d = rng.integers(-4, 5, size=(H, W)).astype(np.int16)
                    d[rng.random((H, W)) < share] = NOMATCH
                    mask = np.where(rng.random((H, W)) < 0.85, 255, rng.integers(0, 255, size=(H, W))).astype(np.uint8)
                    yield Fx(d=d, mask=mask, own=(YL, YR, XL, XR, width, h), W=W, inset=inset, share=share)


def median_counts_map():
    """Negative disparities, half of them NOMATCH: every valid count of the two-column window, centre valid or not."""
    rng = np.random.default_rng(5)
    H, W = 12, 270
    d = rng.integers(-9, 0, size=(H, W)).astype(np.int16)
    d[rng.random((H, W)) < 0.5] = NOMATCH
    d[5, 100:140] = NOMATCH
    d[4:7, 119:121] = NOMATCH                       # k = 0
    d[8:11, 200:206] = rng.integers(-9, 0, size=(3, 6))   # k = 6
    return Fx(d=d, mask=np.full((H, W), 255, np.uint8), own=(1, H - 2, 1, W - 2, W - 2, H - 2))
