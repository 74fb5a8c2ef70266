"""What the Poisson surface says when it refuses a call (csrc/rsm_poisson.hip): the four calls rsm_poisson_mesh{,_weighted,_banded,
_banded_weighted} through both entries (host, _device) and the eight stage entries.  The entries share one host path; the texts below are
written out as the library has always said them, status and whole string, and the double faults pin the order of the checks: params
before n before pointers; the banded call's p NULL, bp NULL, depth, the coarse params, band_bricks, max_iterations, trim_cells; the banded
density call's band checks before dp NULL before the depth - 1 kernel-depth range before the plain density checks.  Dense depth 5, banded
depth 6; nothing is meshed beyond one unspoilt call per entry."""
import ctypes as C

import numpy as np
import pytest
import torch

import poisson_restatement as pr

pytestmark = pytest.mark.gpu

NAN = float("nan")
T_P = "poisson: params is NULL"
T_BP = "poisson: band params is NULL"
T_DP = "poisson: density params is NULL"
T_NULL = "poisson: a NULL pointer"
T_N = "poisson: n -1 outside 0..INT32_MAX"
T_SCALE = "poisson: scale 0.5 not finite or < 1"
T_REL = "poisson: rel_residual 0 not in (0, 1)"
T_CYC = "poisson: max_cycles 0 < 1"
T_TRIM = "poisson: trim_cells -1 < 0"
T_BRICKS = "poisson: band_bricks 0 outside 1..4"
T_ITS = "poisson: max_iterations 0 < 1"
T_TRIM8 = "poisson: trim_cells 8 > 8 band_bricks - 1 = 7 (a kept face needs its cell in the band)"
T_SPN = "poisson: samples_per_node 0 not finite or <= 0"
T_KD_BAND = "poisson: kernel_depth %d neither 0 nor in 3..5 (the banded call's density grid exists at depth - 1 too)"
T_DEPTH_IN = "poisson: depth_in[3] is not finite"
T_GRID = "poisson: iso or grid not finite, or h <= 0"
T_MAXB = "poisson: max_bricks -1 outside 0..2^20"
T_ROOM = "poisson: brick_room -1 < 0"
T_NB = "poisson: n_bricks -1 outside 0..min(B^3, 2^20)"

# what every call with rsm_poisson_params refuses in them, dense (depth 5) ...
DENSE_PARAMS = (
    (dict(p=None), T_P),
    (dict(depth=4), "poisson: depth 4 outside 5..9"),
    (dict(depth=10), "poisson: depth 10 outside 5..9"),
    (dict(scale=0.5), T_SCALE),
    (dict(rel_residual=0.0), T_REL),
    (dict(max_cycles=0), T_CYC),
    (dict(trim_cells=-1), T_TRIM),
    (dict(depth=4, scale=0.5), "poisson: depth 4 outside 5..9"),
    (dict(scale=0.5, rel_residual=0.0), T_SCALE),
    (dict(rel_residual=0.0, max_cycles=0), T_REL),
    (dict(max_cycles=0, trim_cells=-1), T_CYC),
)
# ... and banded (depth 6), each fault with the next one in the order of the checks
BAND_PARAMS = (
    (dict(p=None), T_P),
    (dict(bp=None), T_BP),
    (dict(depth=5), "poisson: banded depth 5 outside 6..10"),
    (dict(depth=11), "poisson: banded depth 11 outside 6..10"),
    (dict(scale=0.5), T_SCALE),
    (dict(rel_residual=0.0), T_REL),
    (dict(max_cycles=0), T_CYC),
    (dict(trim_cells=-1), T_TRIM),
    (dict(band_bricks=0), T_BRICKS),
    (dict(band_bricks=5), "poisson: band_bricks 5 outside 1..4"),
    (dict(max_iterations=0), T_ITS),
    (dict(trim_cells=8), T_TRIM8),
    (dict(p=None, bp=None), T_P),
    (dict(bp=None, depth=5), T_BP),
    (dict(depth=5, scale=0.5), "poisson: banded depth 5 outside 6..10"),
    (dict(scale=0.5, band_bricks=0), T_SCALE),
    (dict(trim_cells=-1, band_bricks=0), T_TRIM),
    (dict(band_bricks=0, max_iterations=0), T_BRICKS),
    (dict(max_iterations=0, trim_cells=8), T_ITS),
)
DENSE_DENSITY = (
    (dict(dp=None), T_DP),
    (dict(kernel_depth=2), "poisson: kernel_depth 2 neither 0 nor in 3..5"),
    (dict(kernel_depth=6), "poisson: kernel_depth 6 neither 0 nor in 3..5"),
    (dict(samples_per_node=0.0), T_SPN),
    (dict(samples_per_node=NAN), "poisson: samples_per_node nan not finite or <= 0"),
    (dict(trim_cells=-1, dp=None), T_TRIM),
    (dict(kernel_depth=6, samples_per_node=0.0), "poisson: kernel_depth 6 neither 0 nor in 3..5"),
    (dict(dp=None, n=-1), T_DP),
    (dict(samples_per_node=0.0, n=-1), T_SPN),
)
BAND_DENSITY = (
    (dict(dp=None), T_DP),
    (dict(kernel_depth=2), T_KD_BAND % 2),
    (dict(kernel_depth=6), T_KD_BAND % 6),
    (dict(samples_per_node=0.0), T_SPN),
    (dict(trim_cells=8, dp=None), T_TRIM8),
    (dict(max_iterations=0, dp=None), T_ITS),
    (dict(bp=None, dp=None), T_BP),
    (dict(dp=None, n=-1), T_DP),
    (dict(kernel_depth=6, samples_per_node=0.0), T_KD_BAND % 6),
    (dict(samples_per_node=0.0, n=-1), T_SPN),
)
# after the params: n, then the pointers
SAMPLES = (
    (dict(n=-1), T_N),
    (dict(xyz=None), T_NULL),
    (dict(nrm=None), T_NULL),
    (dict(trim_cells=-1, n=-1), T_TRIM),
    (dict(n=-1, xyz=None), T_N),
)
CASES = {
    "": DENSE_PARAMS + SAMPLES,
    "_weighted": DENSE_PARAMS + DENSE_DENSITY + SAMPLES,
    "_banded": BAND_PARAMS + SAMPLES + ((dict(trim_cells=8, n=-1), T_TRIM8),),
    "_banded_weighted": BAND_PARAMS + BAND_DENSITY + SAMPLES,
}


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def cloud():
    xyz, nrm = pr.sphere_samples(2000)
    return {"host": (xyz, nrm), "device": (torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda())}


class _Call:
    """the arguments of one call with what a case spoils: sp[key] replaces the default, None makes a pointer NULL"""

    def __init__(self, ctx, cloud, banded, sp):
        from reconstruction_amd._lib import PoissonBandParams, PoissonDensityParams, PoissonParams
        self.lib, self.h, self.sp = ctx._lib, ctx._h, sp
        g = sp.get
        self.prm = PoissonParams(g("depth", 6 if banded else 5), g("scale", 1.1), g("rel_residual", 4e-5), g("max_cycles", 100), g("trim_cells", 2))
        self.bprm = PoissonBandParams(g("band_bricks", 1), g("max_iterations", 200))
        self.dprm = PoissonDensityParams(g("kernel_depth", 0), g("samples_per_node", 2.0))
        self.p = None if "p" in sp else C.byref(self.prm)
        self.bp = None if "bp" in sp else C.byref(self.bprm)
        self.dp = None if "dp" in sp else C.byref(self.dprm)
        self.n = C.c_int64(g("n", 2000))
        self.cloud = cloud

    def samples(self, entry):
        if entry == "device":
            x, m = (C.c_void_p(t.data_ptr()) for t in self.cloud["device"])
        else:
            x, m = (_vp(a) for a in self.cloud["host"])
        return (None if "xyz" in self.sp else x, None if "nrm" in self.sp else m, self.n)

    def out(self, name, a):
        """a host output buffer, NULL when the case names it"""
        return None if name in self.sp else _vp(a)

    def done(self, st):
        return st, (self.lib.rsm_last_error(self.h) or b"").decode()


def _mesh_call(ctx, cloud, kind, entry, **sp):
    a = _Call(ctx, cloud, "banded" in kind, sp)
    nv, nf = C.c_int64(), C.c_int64()
    fn = getattr(a.lib, "rsm_poisson_mesh%s%s" % (kind, "_device" if entry == "device" else ""))
    extra = {"": (), "_weighted": (a.dp,), "_banded": (a.bp,), "_banded_weighted": (a.bp, a.dp)}[kind]
    return a.done(fn(a.h, *a.samples(entry), a.p, *extra, None if "pnv" in sp else C.byref(nv), None if "pnf" in sp else C.byref(nf), None))


@pytest.mark.parametrize("kind", ("", "_weighted", "_banded", "_banded_weighted"))
def test_mesh_calls_refuse_as_they_always_did(ctx, cloud, kind):
    from reconstruction_amd._lib import RSM_E_INVALID
    for entry in ("host", "device"):
        assert _mesh_call(ctx, cloud, kind, entry)[0] in (0, 1), (kind, entry)     # the unspoilt call is taken (1: a solve ended above rel_residual)
        for sp, text in CASES[kind] + ((dict(pnv=None), T_NULL), (dict(pnf=None), T_NULL), (dict(n=-1, pnv=None), T_N)):
            st, msg = _mesh_call(ctx, cloud, kind, entry, **sp)
            assert (st, msg) == (RSM_E_INVALID, text), (kind, entry, sp, st, msg)


def _rhs_call(ctx, cloud, weighted, **sp):
    """rsm_stage_poisson_rhs / _rhs_weighted at depth 5"""
    a = _Call(ctx, cloud, False, sp)
    N3, n = 32 ** 3, 2000
    grid, b, occ, counts = np.zeros(4), np.zeros(N3), np.zeros(N3, np.uint8), np.zeros(2, np.int64)
    outs = (a.out("grid", grid), a.out("b", b), a.out("occ", occ), a.out("counts", counts))
    if not weighted:
        return a.done(a.lib.rsm_stage_poisson_rhs(a.h, *a.samples("host"), a.p, *outs))
    din = sp.get("depth_in")
    rho, w, d = np.zeros(n), np.zeros(n), np.zeros(n)
    return a.done(a.lib.rsm_stage_poisson_rhs_weighted(a.h, *a.samples("host"), a.p, a.dp, _vp(din), *outs, _vp(rho), _vp(w), _vp(d)))


def _bad_depth_in():
    d = np.full(2000, 4.0)
    d[3] = np.inf
    return d


OUTS = tuple((dict([(k, None)]), T_NULL) for k in ("grid", "b", "occ", "counts"))


def test_stage_rhs_refuses_as_it_always_did(ctx, cloud):
    from reconstruction_amd._lib import RSM_E_INVALID
    for weighted in (False, True):
        assert _rhs_call(ctx, cloud, weighted)[0] == 0
        cases = DENSE_PARAMS + SAMPLES + OUTS + ((dict(n=-1, grid=None), T_N),)
        if weighted:
            cases += DENSE_DENSITY + ((dict(depth_in=_bad_depth_in()), T_DEPTH_IN), (dict(depth_in=_bad_depth_in(), grid=None), T_NULL),
                                      (dict(depth_in=_bad_depth_in(), n=-1), T_N))
        for sp, text in cases:
            st, msg = _rhs_call(ctx, cloud, weighted, **sp)
            assert (st, msg) == (RSM_E_INVALID, text), (weighted, sp, st, msg)


def _band_rhs_call(ctx, cloud, weighted, keep=None, **sp):
    """rsm_stage_poisson_band_rhs / _band_rhs_weighted at depth 6; keep: a dict that receives the unspoilt call's outputs"""
    a = _Call(ctx, cloud, True, sp)
    room, n = 512, 2000
    grid, bricks, b = np.zeros(4), np.zeros(room, np.int32), np.zeros(room * 512)
    occ, g, counts = np.zeros(room * 512, np.uint8), np.zeros(room * 512, np.float32), np.zeros(4, np.int64)
    outs = (a.out("grid", grid), a.out("bricks", bricks), a.out("b", b), a.out("occ", occ), a.out("g", g), a.out("counts", counts))
    caps = (None, C.c_int64(sp.get("max_bricks", 0)), C.c_int64(sp.get("brick_room", room)))
    if not weighted:
        st = a.lib.rsm_stage_poisson_band_rhs(a.h, *a.samples("host"), a.p, a.bp, *caps, *outs)
    else:
        rho, w, d = np.zeros(n), np.zeros(n), np.zeros(n)
        st = a.lib.rsm_stage_poisson_band_rhs_weighted(a.h, *a.samples("host"), a.p, a.bp, a.dp, _vp(sp.get("depth_in")), *caps, *outs, _vp(rho), _vp(w), _vp(d))
    if keep is not None:
        keep.update(grid=grid, bricks=bricks, b=b, occ=occ, g=g, counts=counts)
    return a.done(st)


@pytest.fixture(scope="module")
def band(ctx, cloud):
    """the unspoilt band right-hand side at depth 6: its bricks and fields feed the band's solve and extraction entries"""
    keep = {}
    assert _band_rhs_call(ctx, cloud, False, keep=keep)[0] in (0, 1)
    S = int(keep["counts"][2])
    assert 1 < S <= 512
    return dict(S=S, grid=keep["grid"], bricks=keep["bricks"][:S].copy(), b=keep["b"][:S * 512].astype(np.float32), g=keep["g"][:S * 512].copy(),
                occ=keep["occ"][:S * 512].copy())


BAND_OUTS = tuple((dict([(k, None)]), T_NULL) for k in ("grid", "bricks", "b", "occ", "g", "counts"))


def test_stage_band_rhs_refuses_as_it_always_did(ctx, cloud, band):
    from reconstruction_amd._lib import RSM_E_INVALID
    S = band["S"]
    for weighted in (False, True):
        assert _band_rhs_call(ctx, cloud, weighted)[0] in (0, 1)
        cases = BAND_PARAMS + SAMPLES + BAND_OUTS + (
            (dict(max_bricks=-1), T_MAXB),
            (dict(max_bricks=(1 << 20) + 1), "poisson: max_bricks 1048577 outside 0..2^20"),
            (dict(brick_room=-1), T_ROOM),
            (dict(n=-1, max_bricks=-1), T_N),
            (dict(max_bricks=-1, brick_room=-1), T_MAXB),
            (dict(brick_room=-1, grid=None), T_ROOM),
            (dict(max_bricks=1), "poisson: %d active bricks, more than the 1 allowed (such a cloud fills the volume)" % S),
            (dict(brick_room=1), "poisson: %d active bricks, brick_room 1" % S),
            (dict(max_bricks=1, brick_room=1), "poisson: %d active bricks, more than the 1 allowed (such a cloud fills the volume)" % S),
        )
        if weighted:
            cases += BAND_DENSITY + ((dict(depth_in=_bad_depth_in()), T_DEPTH_IN), (dict(depth_in=_bad_depth_in(), grid=None), T_NULL),
                                     (dict(depth_in=_bad_depth_in(), brick_room=-1), T_ROOM))
        for sp, text in cases:
            st, msg = _band_rhs_call(ctx, cloud, weighted, **sp)
            assert (st, msg) == (RSM_E_INVALID, text), (weighted, sp, st, msg)


def _solve_call(ctx, b32, **sp):
    """rsm_stage_poisson_solve at depth 5"""
    g = sp.get
    chi, res, cyc = np.zeros(32 ** 3, np.float32), C.c_double(), C.c_int()
    st = ctx._lib.rsm_stage_poisson_solve(ctx._h, None if "b" in sp else _vp(b32), g("depth", 5), g("rel_residual", 4e-5), g("max_cycles", 100),
                                          None if "chi" in sp else _vp(chi), None if "res" in sp else C.byref(res), None if "cyc" in sp else C.byref(cyc), None)
    return (st, (ctx._lib.rsm_last_error(ctx._h) or b"").decode()), chi


def _iso_call(ctx, chi32, grid4, occ8, **sp):
    """rsm_stage_iso_mesh at depth 5"""
    g = sp.get
    nv, nf = C.c_int64(), C.c_int64()
    grid4 = g("grid_values", grid4)
    st = ctx._lib.rsm_stage_iso_mesh(ctx._h, None if "chi" in sp else _vp(chi32), g("depth", 5), g("iso", 0.0), None if "grid" in sp else _vp(grid4),
                                     None if "occ" in sp else _vp(occ8), g("trim_cells", 2), None if "pnv" in sp else C.byref(nv), C.byref(nf))
    return st, (ctx._lib.rsm_last_error(ctx._h) or b"").decode()


def test_stage_solve_and_iso_mesh_refuse_as_they_always_did(ctx, cloud):
    from reconstruction_amd._lib import RSM_E_INVALID
    grid, b, occ, _ = ctx.poisson_rhs(*cloud["host"], 5)
    b32 = np.ascontiguousarray(b, np.float32).ravel()
    (st, _), chi = _solve_call(ctx, b32)
    assert st == 0
    for sp, text in ((dict(depth=4), "poisson: depth 4 outside 5..9"), (dict(rel_residual=0.0), T_REL), (dict(rel_residual=1.0), "poisson: rel_residual 1 not in (0, 1)"),
                     (dict(max_cycles=0), T_CYC), (dict(b=None), T_NULL), (dict(chi=None), T_NULL), (dict(res=None), T_NULL), (dict(cyc=None), T_NULL),
                     (dict(depth=4, rel_residual=0.0), "poisson: depth 4 outside 5..9"), (dict(max_cycles=0, b=None), T_CYC)):
        (st, msg), _ = _solve_call(ctx, b32, **sp)
        assert (st, msg) == (RSM_E_INVALID, text), (sp, st, msg)
    occ = np.ascontiguousarray(occ).ravel()
    assert _iso_call(ctx, chi, grid, occ)[0] == 0
    assert _iso_call(ctx, chi, grid, occ, occ=None, trim_cells=0)[0] == 0          # no trim needs no occupancy
    flat = grid.copy()
    flat[3] = 0.0
    for sp, text in ((dict(depth=10), "poisson: depth 10 outside 5..9"), (dict(trim_cells=-1), T_TRIM), (dict(chi=None), T_NULL), (dict(grid=None), T_NULL),
                     (dict(pnv=None), T_NULL), (dict(occ=None), T_NULL), (dict(iso=NAN), T_GRID), (dict(grid_values=flat), T_GRID),
                     (dict(depth=10, trim_cells=-1), "poisson: depth 10 outside 5..9"), (dict(trim_cells=-1, chi=None), T_TRIM), (dict(pnv=None, iso=NAN), T_NULL)):
        st, msg = _iso_call(ctx, chi, grid, occ, **sp)
        assert (st, msg) == (RSM_E_INVALID, text), (sp, st, msg)


def _list_cases(S):
    """what poisson_band_list_ok refuses, for both entries that take a caller's list"""
    desc, far = np.arange(S, dtype=np.int32), np.arange(S, dtype=np.int32)
    desc[1] = 0
    far[S - 1] = 512
    return ((dict(depth=5), "poisson: banded depth 5 outside 6..10"), (dict(n_bricks=-1), T_NB),
            (dict(n_bricks=513), "poisson: n_bricks 513 outside 0..min(B^3, 2^20)"), (dict(bricks=None), T_NULL),
            (dict(bricks_values=desc), "poisson: bricks[1] = 0 out of range or not ascending"),
            (dict(bricks_values=far), "poisson: bricks[%d] = 512 out of range or not ascending" % (S - 1)),
            (dict(depth=5, n_bricks=-1), "poisson: banded depth 5 outside 6..10"), (dict(n_bricks=-1, bricks=None), T_NB))


def _band_solve_call(ctx, band, **sp):
    g = sp.get
    chi, res, res0, its = np.zeros(band["S"] * 512, np.float32), C.c_double(), C.c_double(), C.c_int()
    bricks = g("bricks_values", band["bricks"])
    st = ctx._lib.rsm_stage_poisson_band_solve(ctx._h, None if "bricks" in sp else _vp(bricks), C.c_int64(g("n_bricks", band["S"])), g("depth", 6),
                                               None if "b" in sp else _vp(band["b"]), None if "g" in sp else _vp(band["g"]), None, g("rel_residual", 4e-5),
                                               g("max_iterations", 200), None if "chi" in sp else _vp(chi), None if "res" in sp else C.byref(res),
                                               None if "its" in sp else C.byref(its), None if "res0" in sp else C.byref(res0), None)
    return (st, (ctx._lib.rsm_last_error(ctx._h) or b"").decode()), chi


def _band_iso_call(ctx, band, chi32, **sp):
    g = sp.get
    nv, nf = C.c_int64(), C.c_int64()
    bricks, grid = g("bricks_values", band["bricks"]), g("grid_values", band["grid"])
    st = ctx._lib.rsm_stage_band_iso_mesh(ctx._h, None if "bricks" in sp else _vp(bricks), C.c_int64(g("n_bricks", band["S"])), g("depth", 6),
                                          None if "chi" in sp else _vp(chi32), g("iso", 0.0), None if "grid" in sp else _vp(grid),
                                          None if "occ" in sp else _vp(band["occ"]), g("trim_cells", 2), None if "pnv" in sp else C.byref(nv), C.byref(nf))
    return st, (ctx._lib.rsm_last_error(ctx._h) or b"").decode()


def test_stage_band_solve_and_iso_mesh_refuse_as_they_always_did(ctx, band):
    from reconstruction_amd._lib import RSM_E_INVALID
    (st, _), chi = _band_solve_call(ctx, band)
    assert st in (0, 1)                                                            # (without a coarse field the solve may end above rel_residual)
    for sp, text in _list_cases(band["S"]) + (
            (dict(rel_residual=0.0), T_REL), (dict(max_iterations=0), T_ITS), (dict(b=None), T_NULL), (dict(g=None), T_NULL), (dict(chi=None), T_NULL),
            (dict(res=None), T_NULL), (dict(its=None), T_NULL), (dict(res0=None), T_NULL), (dict(n_bricks=-1, rel_residual=0.0), T_NB),
            (dict(rel_residual=0.0, max_iterations=0), T_REL), (dict(max_iterations=0, res=None), T_ITS)):
        (st, msg), _ = _band_solve_call(ctx, band, **sp)
        assert (st, msg) == (RSM_E_INVALID, text), (sp, st, msg)
    assert _band_iso_call(ctx, band, chi)[0] == 0
    flat = band["grid"].copy()
    flat[3] = 0.0
    for sp, text in _list_cases(band["S"]) + (
            (dict(trim_cells=-1), T_TRIM), (dict(chi=None), T_NULL), (dict(grid=None), T_NULL), (dict(pnv=None), T_NULL), (dict(occ=None), T_NULL),
            (dict(iso=NAN), T_GRID), (dict(grid_values=flat), T_GRID), (dict(n_bricks=-1, trim_cells=-1), T_NB), (dict(trim_cells=-1, chi=None), T_TRIM),
            (dict(pnv=None, iso=NAN), T_NULL)):
        st, msg = _band_iso_call(ctx, band, chi, **sp)
        assert (st, msg) == (RSM_E_INVALID, text), (sp, st, msg)
