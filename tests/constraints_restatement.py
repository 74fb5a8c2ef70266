"""The integer constraint stages of MatchOneLayer restated from the reference's text, in the reference's own form: plain
Python / numpy, serial where the reference is serial, with its scatter, its dense crossing matrix and its sorted median.

    uniqueness_pass    CStereoMatching::UniquenessContraint_<T>   .cpp:463-497
    order_constraint   CStereoMatching::OrderConstraint           .cpp:310-368
    smooth_constraint  CStereoMatching::SmoothConstraint          .cpp:370-448
    median_filter      CStereoMatching::MedianFilter              .cpp:763-815

Nothing here is shared with oracle/ (C, counts without the matrix) or with the kernels (gather form, carry chains, components,
sorting network): the module imports numpy and nothing of the project.  tests/test_constraints_cpu.py holds it to the oracle;
tests/test_gpu_constraint_chains.py holds the kernels to both."""
import numpy as np

NOMATCH = -10000


def _margin(own):
    return int(own[0]), int(own[1]), int(own[2]), int(own[3])


# ---------------------------------------------------------------- UniquenessContraint_<T>
# classes of a pixel of the own margin, as the serial loop meets it
INVALID, DIRECT, BY_NEXT, BY_PREV, CHAIN_KILLED, KILLED = 0, 1, 2, 3, 4, 5


def uniqueness_pass(p, q, own, oth):
    """One pass of .cpp:474-496 over p (int16 or float64; q of the same type).  Returns (new p, cls, run):

    cls   0 invalid; 1 kept by a direct match (:487); 2 kept by p[x+1] (:492, second test); 3 kept only by a LIVE p[x-1]
          (first test of :492, read after the loop may have killed it); 4 killed although |q[bL+1] + p[x-1]| < 2 held on the
          input, because p[x-1] had been killed; 5 killed otherwise.  (With q[bL+1] within 2 of +10000 the first test holds
          against a p[x-1] that reads NOMATCH: class 3 then means kept by what p[x-1] reads, dead or never valid.)
    run   for class 3 the length of the run of class-3 pixels ending at the pixel, else 0.

    p and q are cv::Mat rows: T* into one flat buffer.  q[boundary_L+1] is not confined to [XL1, XR1] nor to the row: past the
    row's end it reads the next row, and beyond the buffer the oracle defines the read as NOMATCH (the reference reads the
    heap there)."""
    p = np.array(p)
    flt = p.dtype == np.float64
    q = np.ascontiguousarray(q, p.dtype)
    H, W = p.shape
    YL, YR, XL, XR = _margin(own)
    XL1, XR1 = int(oth[2]), int(oth[3])
    orig = [v.item() for v in p.ravel()]
    cur = list(orig)
    qf = [v.item() for v in q.ravel()]
    total = W * H
    cls = np.zeros((H, W), np.int8)
    run = np.zeros((H, W), np.int32)

    def flat(buf, i):
        return buf[i] if 0 <= i < total else NOMATCH

    for y in range(YL, YR + 1):
        row = y * W
        for x in range(XL, XR + 1):
            px = cur[row + x]
            if px == NOMATCH:
                continue
            bl = max(int(px + 0.5) + x - 1, XL1)          # :482 -- int() truncates towards zero, as the C cast does
            br = min(bl + 2, XR1)
            i = bl
            while i <= br:
                if abs(qf[row + i] + px) < 2:
                    break
                i += 1
            if i <= br:
                cls[y, x] = DIRECT
                continue
            qv = flat(qf, row + bl + 1)
            by_prev = abs(qv + flat(cur, row + x - 1)) < 2
            by_next = abs(qv + flat(cur, row + x + 1)) < 2
            if by_next:
                cls[y, x] = BY_NEXT
            elif by_prev:
                cls[y, x] = BY_PREV
                run[y, x] = (run[y, x - 1] if x > XL and cls[y, x - 1] == BY_PREV else 0) + 1
            else:
                cur[row + x] = NOMATCH                    # :493
                was = abs(qv + flat(orig, row + x - 1)) < 2
                cls[y, x] = CHAIN_KILLED if was else KILLED
    out = np.array(cur, dtype=p.dtype).reshape(H, W)
    return out, cls, run


def uniqueness(d0, d1, m0, m1):
    """UniquenessContraint<T> (.cpp:450-461): (d0 | d1), (d1 | d0), (d0 | d1)."""
    d0 = uniqueness_pass(d0, d1, m0, m1)[0]
    d1 = uniqueness_pass(d1, d0, m1, m0)[0]
    d0 = uniqueness_pass(d0, d1, m0, m1)[0]
    return d0, d1


# ---------------------------------------------------------------- OrderConstraint
def order_constraint(d, own, stats=None):
    """.cpp:321-367 per row with the dense matrix A of :337-351.  If `stats` is a list, one dict per row is appended to it:
    n valid pixels, removed, and -- from A's own structure, a cut being a list position no crossing pair straddles --
    the number of components that hold a crossing, the longest component, the list positions at which components end,
    and pmax - pmin over the valid disparities."""
    d = np.array(d, dtype=np.int16)
    YL, YR, XL, XR = _margin(own)
    for y in range(YL, YR + 1):
        p = d[y]
        index = [x for x in range(XL, XR + 1) if p[x] != NOMATCH]            # :328-335
        line = np.array([int(p[x]) + x for x in index], dtype=np.int64).astype(np.int16)
        n = len(index)
        A = np.zeros((n, n), np.int16)
        if n:
            i, j = np.tril_indices(n, -1)
            A[i, j] = line[j] > line[i]                                       # :340-350
        ones_count = int(A.sum(dtype=np.int64))
        A = A + A.T                                                           # :351
        if stats is not None:
            stats.append(_row_stats(A, [int(p[x]) for x in index]))
        cross_count = A.sum(axis=1, dtype=np.int16)                           # arma::Col<short>
        removed = 0
        while ones_count:                                                     # :354-364
            m = int(np.argmax(cross_count))                                   # the first maximum (op_max scans with '>')
            max_cross = int(cross_count[m])
            cross_count = cross_count - A[:, m]
            cross_count[m] = 0
            A[m, :] = 0
            A[:, m] = 0
            ones_count -= max_cross
            p[index[m]] = NOMATCH
            removed += 1
        if stats is not None:
            stats[-1]["removed"] = removed
    return d


def _row_stats(A, disp):
    n = len(disp)
    if n == 0:
        return dict(n=0, components=0, longest=0, ends=[], spread=0)
    # position i is a cut iff no pair j <= i < k crosses
    cut = [not A[:i + 1, i + 1:].any() for i in range(n)]
    ends = [i for i in range(n) if cut[i]]
    comps, longest, start = 0, 0, 0
    for e in ends:
        longest = max(longest, e - start + 1)
        comps += bool(A[start:e + 1, start:e + 1].any())
        start = e + 1
    return dict(n=n, components=comps, longest=longest, ends=ends, spread=max(disp) - min(disp))


# ---------------------------------------------------------------- SmoothConstraint
def smooth_constraint(d, own):
    """.cpp:379-447: the serial scatter into a CV_8UC2 map (uchar counters: total, differing), the south-east totals at BYTE
    index x and x + 2 (:423-424, not 2x and 2x + 2), then the kill rule of :443.  Needs the margin at least one pixel inside
    the image, which is what FindMargin gives."""
    d = np.array(d, dtype=np.int16)
    H, W = d.shape
    YL, YR, XL, XR = _margin(own)
    assert 1 <= XL and XR <= W - 2 and 0 <= YL and YR <= H - 2
    P = d.tolist()
    temp = [[0] * (2 * W) for _ in range(H)]                                   # :379

    def inc(row, i):
        row[i] = (row[i] + 1) & 255                                           # uchar ++

    def differ(a, b):                                                         # DifferOfDisparity, :3
        return abs(a - b) > 1

    for y in range(YL, YR + 1):
        pup, pdown = P[y], P[y + 1]
        qup, qdown = temp[y], temp[y + 1]
        for x in range(XL, XR + 1):
            if pup[x] == NOMATCH:
                continue
            dx = x << 1
            if pup[x + 1] != NOMATCH:                                         # east
                inc(qup, dx); inc(qup, dx + 2)
                if differ(pup[x], pup[x + 1]):
                    inc(qup, dx + 1); inc(qup, dx + 3)
            if pdown[x - 1] != NOMATCH:                                       # south-west
                inc(qup, dx); inc(qdown, dx - 2)
                if differ(pup[x], pdown[x - 1]):
                    inc(qup, dx + 1); inc(qdown, dx - 1)
            if pdown[x] != NOMATCH:                                           # south
                inc(qup, dx); inc(qdown, dx)
                if differ(pup[x], pdown[x]):
                    inc(qup, dx + 1); inc(qdown, dx + 1)
            if pdown[x + 1] != NOMATCH:                                       # south-east
                inc(qup, x); inc(qdown, x + 2)                                # :423-424, as written
                if differ(pup[x], pdown[x + 1]):
                    inc(qup, dx + 1); inc(qdown, dx + 3)
    for y in range(YL, YR + 1):                                               # :435-447
        chk = temp[y]
        for x in range(XL, XR + 1):
            if chk[2 * x] == 0 or (chk[2 * x + 1] << 1) > chk[2 * x]:
                d[y, x] = NOMATCH
    return d


# ---------------------------------------------------------------- MedianFilter (one iteration)
def arma_median(u):
    """arma::median of an ivec: sorted middle; for an even count lo + (hi - lo) / 2 in C's integer division."""
    u = sorted(u)
    half = len(u) // 2
    if len(u) % 2:
        return u[half]
    lo, hi = u[half - 1], u[half]
    diff = hi - lo
    return lo + (abs(diff) // 2) * (1 if diff >= 0 else -1)                   # C division truncates towards zero


def median_filter(d, mask, own, counts=None):
    """.cpp:772-813.  If `counts` is an int array of d's shape, the k of :792-795 is stored for every pixel visited."""
    d = np.asarray(d, dtype=np.int16)
    mask = np.asarray(mask)
    YL, YR, XL, XR = _margin(own)
    out = np.full(d.shape, NOMATCH, np.int16)                                 # :772
    P = d.tolist()
    for y in range(YL, YR + 1):
        window = [P[y - 1], P[y], P[y + 1]]
        for x in range(XL, XR + 1):
            if mask[y, x] != 255:
                continue
            u = []
            for i in range(x - 1, x + 1):                                     # :792 -- columns x-1 and x
                for j in range(3):
                    if window[j][i] != NOMATCH:
                        u.append(window[j][i])
            k = len(u)
            if counts is not None:
                counts[y, x] = k
            if window[1][x] == NOMATCH:
                out[y, x] = arma_median(u) if k >= 4 else NOMATCH
            else:
                out[y, x] = NOMATCH if k <= 2 else arma_median(u)
    return out
