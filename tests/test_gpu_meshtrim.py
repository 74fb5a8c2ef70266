"""GPU density trim of the Poisson surface (csrc/k_meshtrim.hip) against the numpy restatement
(tests/meshtrim_restatement.py).  rho is the same bits (an integer splat and eight fp64 terms in a fixed order); value may differ through
the two log2 implementations alone and is held to 1e-12 (a couple of ulps of a number below 64 are 3e-14: a cap, not a measurement);
everything after the value is computed from caller-supplied values and is exact -- smoothed values, split vertices, faces, sides, labels,
counts.  If bits differ, look for a contracted multiply-add or another order of summation; the comparison is not to be loosened."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import meshclean_restatement as mr
import meshtrim_restatement as mt
import poisson_restatement as pr
from reconstruction_amd import synth

pytestmark = pytest.mark.gpu

INT_KEYS = mt.STAT_KEYS


def ints(stats):
    return {k: stats[k] for k in INT_KEYS}


# ---- 1: density ---------------------------------------------------------------------------------------------------------------------------
def cap_with_bad_samples():
    xyz, nrm = mt.cap_samples()
    xyz, nrm = xyz.copy(), nrm.copy()
    xyz[17, 1] = np.nan            # no sample either way
    nrm[40, :3] = 0.0              # a sample only without normals
    return xyz, nrm


@pytest.mark.parametrize("kernel_depth", [3, 5])
@pytest.mark.parametrize("with_normals", [True, False])
def test_density_is_the_restatements_bits_and_value_within_the_log2_cap(ctx, kernel_depth, with_normals):
    xyz, nrm = cap_with_bad_samples()
    n4 = nrm if with_normals else None
    p, _ = mt.valid_points(xyz, n4)
    o, hk = mt.density_grid(p, 5, 1.0, kernel_depth)
    side = hk * (1 << kernel_depth)
    far_face = o + np.array([side, 0.5 * side, 0.5 * side])                    # on the last node's far face (scale = 1: also the box's)
    pts = np.concatenate([xyz[:400:2], xyz[:1] + 0.37 * hk, [o - 10.0 * side], [far_face], [o + side - 1e-3], [pr.SPHERE_C], [o + 0.5 * hk]]).astype(np.float32)
    pts = pts[np.isfinite(pts).all(1)]
    want_rho, want_val, want_counts = mt.density(xyz, n4, pts, 5, 1.0, kernel_depth)
    rho, val, counts = ctx.mesh_density(xyz, n4, pts, 5, 1.0, kernel_depth)
    diff = np.abs(val - want_val).max()
    print("kernel depth %d, normals %d: %d points, rho bits differing %d, max |value - restatement| %.3g, rho %.3g .. %.3g"
          % (kernel_depth, with_normals, len(pts), int((rho.view(np.uint64) != want_rho.view(np.uint64)).sum()), diff, rho.min(), rho.max()))
    assert counts == want_counts == ((1992, 2) if with_normals else (1993, 1))
    assert rho.tobytes() == want_rho.tobytes()
    assert diff <= 1e-12 and np.array_equal(val == 0.0, want_val == 0.0)
    assert rho[-5] == 0.0 and val[-5] == 0.0                                    # outside the grid
    assert rho[-2] == 0.0                                                       # the empty region around the sphere's centre
    assert (rho[:200] > 0).sum() >= 199 and val.max() > 4.0                     # (the sample whose normal is zero may stand alone)


def test_no_valid_sample_gives_value_zero_everywhere(ctx):
    pts = np.float32([[0, 0, 0], [1, 2, 3]])
    for xyz in (np.full((5, 3), np.nan, np.float32), np.zeros((0, 3), np.float32), np.ones((4, 3), np.float32)):   # none finite, none at all, all equal
        rho, val, counts = ctx.mesh_density(xyz, None, pts, 5)
        assert not rho.any() and not val.any() and counts == mt.density(xyz, None, pts, 5)[2]


# ---- 2: value smoothing, the same bits -----------------------------------------------------------------------------------------------------
def smoothing_meshes():
    rng = np.random.default_rng(11)
    fan = np.int32([[0, 1, 2], [1, 0, 3], [0, 1, 4]])                            # three faces on the edge (0, 1)
    pv, pf = mt.plane(4, 4)
    odd = np.concatenate([pf, np.int32([[5, 5, 6], [2, 9, 2]])])                 # repeated indices; vertex 16 is in no face
    soup = rng.integers(0, 257, size=(600, 3)).astype(np.int32)
    return {"triangle": (3, np.int32([[0, 1, 2]])), "plane": (41 * 31, mt.plane(41, 31)[1]), "three_face_edge": (5, fan), "repeated_unreferenced": (17, odd),
            "soup": (257, soup)}


@pytest.mark.parametrize("name", ["triangle", "plane", "three_face_edge", "repeated_unreferenced", "soup"])
def test_value_smoothing_is_the_restatements_bits(ctx, name):
    nv, f = smoothing_meshes()[name]
    x = np.random.default_rng(5).normal(7.0, 2.0, size=nv)
    for steps in (0, 1, 2, 100):
        got, want = ctx.mesh_value_smooth(x, f, steps), mt.value_smooth(x, f, steps)
        print("%s, %d steps: values whose bits differ: %d of %d" % (name, steps, int((got.view(np.uint64) != want.view(np.uint64)).sum()), nv))
        assert got.tobytes() == want.tobytes()
    assert ctx.mesh_value_smooth(x, f, 0).tobytes() == x.tobytes()
    if name == "repeated_unreferenced":
        assert got[16] == x[16]
    if name != "triangle":
        assert not np.array_equal(got, ctx.mesh_value_smooth(x, f, 2))


# ---- 3: split -----------------------------------------------------------------------------------------------------------------------------
def split_scenes():
    rng = np.random.default_rng(3)
    out = {}
    for flip in (False, True):
        v, f = mt.plane(13, 11, flip=flip)
        out["random_flip%d" % flip] = (v, f, rng.uniform(5.0, 9.0, size=len(v)), True)
    v, f = mt.plane(13, 11)
    out["integers"] = (v, f, rng.integers(5, 10, size=len(v)).astype(np.float64), True)
    v, f = mt.tetra_sphere(3)
    out["sphere"] = (v, f, 7.013 + 2.0 * v[:, 2].astype(np.float64) + 0.3 * v[:, 0].astype(np.float64), True)
    v = np.float32([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0], [0.5, 0, 1]])
    out["three_face_edge"] = (v, np.int32([[0, 1, 2], [1, 0, 3], [0, 1, 4]]), np.float64([8.0, 6.0, 6.5, 7.5, 6.0]), False)
    return out


def same_border_line(a, b, lo, hi):
    return any((a[k] == b[k]) and (a[k] == lo[k] or a[k] == hi[k]) for k in range(2))


@pytest.mark.parametrize("name", ["random_flip0", "random_flip1", "integers", "sphere", "three_face_edge"])
def test_split_is_the_restatements_mesh_and_is_closed_off_the_cut(ctx, name):
    v, f, x, manifold = split_scenes()[name]
    want = mt.split(v, f, x, 7.0, 0.0)
    ov, of, src, side, label, st = ctx.mesh_split(v, f, x, 7.0, 0.0)
    print("%s: %d faces -> %d (%d split, %d cut edges, %d zero-area triangles)" % (name, len(f), len(of), st["faces_split"], st["cut_edges"], st["zero_area_triangles"]))
    assert ov.tobytes() == want["vertices"].tobytes() and np.array_equal(of, want["faces"])
    assert np.array_equal(src, want["src"]) and np.array_equal(side, want["side"]) and np.array_equal(label, want["label"])
    assert ints(st) == want["stats"] and st["diagonal2"] == want["D2"] and st["value_min"] == x.min() and st["value_max"] == x.max()
    assert (side == 1).all() and st["moved_to_kept"] == 0 and len(of) > 0
    keep = x >= 7.0
    if name.startswith("random"):                                                # all eight keep patterns
        assert len({tuple(k) for k in keep[f].tolist()}) == 8
    if name == "integers":                                                       # t = 0 and t = 1 both occur, with their zero-area triangles
        assert (x == 7.0).any() and st["zero_area_triangles"] > 0
        lo_, hi_ = want["cut_keys"] >> 32, want["cut_keys"] & 0xffffffff
        assert (x[lo_] == 7.0).any() and (x[hi_] == 7.0).any()
    if not manifold:                                                             # the shared edge (0, 1) is cut once; its vertex, the lowest key's, serves all three faces
        assert st["cut_edges"] == 4 and st["faces_split"] == 3
        n_orig = int((np.unique(want["split_faces"][want["split_final"] == 1]) < len(v)).sum())
        assert {int(s_) for s_, t in zip(src, of) if n_orig in t.tolist()} == {0, 1, 2}
        return
    # off the cut line and off the input's border every edge lies in two faces, once per direction
    n_orig = int((np.unique(want["split_faces"][want["split_final"] == 1]) < len(v)).sum())
    lo, hi = v.min(0), v.max(0)
    directed = {}
    for t in of.tolist():
        for j in range(3):
            directed[(t[j], t[(j + 1) % 3])] = directed.get((t[j], t[(j + 1) % 3]), 0) + 1
    assert set(directed.values()) == {1}
    open_edges = [(a, b) for (a, b) in directed if (b, a) not in directed]
    for a, b in open_edges:
        on_cut = a >= n_orig and b >= n_orig
        on_border = name != "sphere" and same_border_line(ov[a], ov[b], lo, hi)
        assert on_cut or on_border, (a, b, ov[a], ov[b])
    assert any(a >= n_orig and b >= n_orig for a, b in open_edges)
    # one vertex per cut edge, used by the kept pieces of both faces on it
    crossing = {(min(a, b), max(a, b)) for t in f.tolist() for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])) if keep[a] != keep[b]}
    assert st["cut_edges"] == len(crossing) == len(want["cut_keys"])
    used_split = np.unique(want["split_faces"][want["split_final"] == 1])
    faces_on = {}
    for fi, t in enumerate(f.tolist()):
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            faces_on.setdefault((min(a, b) << 32) | max(a, b), set()).add(fi)
    users = {}
    for s, t in zip(src.tolist(), of.tolist()):
        for q in t:
            if q >= n_orig:
                users.setdefault(q, set()).add(s)
    cut_ids = used_split[used_split >= len(v)] - len(v)
    assert len(cut_ids) == len(users) == len(want["cut_keys"])
    for out_id, r in zip(range(n_orig, n_orig + len(cut_ids)), cut_ids):
        assert users[out_id] == faces_on[int(want["cut_keys"][r])]


# ---- 4: islands ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.01, 0.0])
def test_islands_are_the_restatements(ctx, ratio):
    V, F, val, names, want = mt.island_result(ratio)
    for c, q in want["Q"].items():                                               # no component near the threshold: a last-bit difference cannot decide
        assert abs(q / (0.01 * want["stats"]["q_total"]) - 1.0) > 0.01
    ov, of, src, side, label, st = ctx.mesh_split(V, F, val, 7.0, ratio)
    print("ratio %g: %s" % (ratio, st))
    assert ints(st) == want["stats"]
    assert ov.tobytes() == want["vertices"].tobytes() and np.array_equal(of, want["faces"])
    assert np.array_equal(src, want["src"]) and np.array_equal(side, want["side"]) and np.array_equal(label, want["label"])
    assert (st["moved_to_kept"], st["moved_to_dropped"]) == ((1, 1) if ratio else (0, 0))
    c = ov[of].mean(1)
    near = lambda p, r: int(((c[:, 0] - p[0]) ** 2 + (c[:, 1] - p[1]) ** 2 < r * r).sum())
    assert (near(names["small_low_disc"], 1.5) > 0) == bool(ratio) and near(names["big_low_disc"], 1.5) == 0
    assert (near(names["small_high_disc"], 1.5) == 0) == bool(ratio)
    assert near(names["high_sphere"], 2.5) == 64 and near(names["low_sphere"], 2.5) == 0
    assert (0 in side.tolist()) == bool(ratio)                                   # the filled-back disc comes from the dropped side


# ---- 5: the whole call ----------------------------------------------------------------------------------------------------------------------
WHOLE = dict(depth=5, scale=1.1, kernel_depth=0, samples_per_node=2.0, smooth_steps=10, trim=5.0, island_ratio=0.01)


def border_vertices(f, nv):
    return mr.incidences(f, nv)[1]


def test_whole_call_is_the_restatement_on_the_gpus_values_and_all_entries_agree(ctx):
    xyz, nrm = mt.cap_samples()
    pv, pf, pst = ctx.poisson_mesh(xyz, nrm, 5, trim_cells=0)
    # the unclipped surface has no border inside the box: what border it has lies on the lattice's outer planes
    o, h, N = np.array(pst["origin"]), pst["h"], pst["N"]
    b0 = border_vertices(pf, len(pv))
    on_wall = (np.minimum(np.abs(pv - (o + 0.5 * h)), np.abs(pv - (o + (N - 0.5) * h))).min(1) < 1e-3 * h)
    assert len(pf) > 1000 and on_wall[b0].all()
    v1, f1, s1 = ctx.mesh_trim_last(xyz, nrm, **WHOLE)
    vals = ctx.mesh_density(xyz, nrm, pv, 5, 1.1)[1]
    want = mt.trim_mesh(pv, pf, xyz, nrm, values=vals, **WHOLE)
    print("whole call: %d faces -> %d; %s" % (len(pf), len(f1), s1))
    assert v1.tobytes() == want["vertices"].tobytes() and np.array_equal(f1, want["faces"]) and ints(s1) == want["stats"]
    assert s1["value_min"] == want["values"].min() and s1["value_max"] == want["values"].max() and s1["kernel_depth"] == 3
    assert 100 < len(f1) < len(pf) and s1["n_valid"] == len(xyz)
    # every border vertex of the result is a cut vertex
    n_orig = int((np.unique(want["split_faces"][want["split_final"] == 1]) < len(pv)).sum())
    b1 = np.nonzero(border_vertices(f1, len(v1)))[0]
    assert len(b1) > 10 and (b1 >= n_orig).all()
    # the last mesh is the result; the host and the device entry give the same bytes, and so does a second run
    hv, hf = ctx.poisson_last_mesh(len(v1), len(f1))
    assert hv.tobytes() == v1.tobytes() and hf.tobytes() == f1.tobytes()
    for _ in range(2):
        v2, f2, s2 = ctx.mesh_trim(pv, pf, xyz, nrm, **WHOLE)
        assert v2.tobytes() == v1.tobytes() and f2.tobytes() == f1.tobytes() and s2 == s1
    dv, df, dx, dn = (torch.from_numpy(a).cuda() for a in (pv, pf, xyz, nrm))
    nv, nf, s3 = ctx.mesh_trim_device(dv.data_ptr(), len(pv), df.data_ptr(), len(pf), dx.data_ptr(), dn.data_ptr(), len(xyz), 5, 1.1,
                                      **{k: WHOLE[k] for k in ("smooth_steps", "trim")})
    assert (nv, nf) == (len(v1), len(f1)) and s3 == s1
    ov = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    of = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    ctx.poisson_last_mesh_device(ov.data_ptr(), of.data_ptr())
    torch.cuda.synchronize()
    assert ov.cpu().numpy().tobytes() == v1.tobytes() and of.cpu().numpy().tobytes() == f1.tobytes()
    # without normals the zero-normal rule is gone, nothing else
    nv4, nf4, s4 = ctx.mesh_trim_device(dv.data_ptr(), len(pv), df.data_ptr(), len(pf), dx.data_ptr(), 0, len(xyz), 5, 1.1, smooth_steps=10, trim=5.0)
    assert (nv4, nf4) == (nv, nf) and s4 == s1


# ---- 6: refusals, the empty mesh ------------------------------------------------------------------------------------------------------------
def test_invalid_input_is_refused_and_named(ctx):
    from reconstruction_amd import RsmError
    from reconstruction_amd._lib import RSM_E_INVALID, MeshTrimParams
    lib, h = ctx._lib, ctx._h
    v, f = mt.plane(5, 5)
    s = np.float32([[0, 0, 0], [4, 4, 1], [2, 1, 0]])
    nv, nf = C.c_int64(), C.c_int64()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(V=v, F=f, S=s, n_v=None, n_f=None, n=None, pn=C.byref(nv), **kw):
        p = MeshTrimParams(5, 1.1, 0, 2.0, 3, 1.0, 0.01)
        for k, val in kw.items():
            setattr(p, k, val)
        st = lib.rsm_mesh_trim(h, ptr(V), C.c_int64(len(V) if n_v is None else n_v), ptr(F), C.c_int64(len(F) if n_f is None else n_f), ptr(S), None,
                               C.c_int64(len(S) if n is None else n), C.byref(p), pn, C.byref(nf), None)
        return st, (lib.rsm_last_error(h) or b"").decode()
    bad_i, neg_i, bad_c = f.copy(), f.copy(), v.copy()
    bad_i[7, 1] = len(v)
    neg_i[0, 0] = -1
    bad_c[3, 2] = np.nan
    nan, inf = float("nan"), float("inf")
    for kw, name in ((dict(depth=4), "depth"), (dict(depth=10), "depth"), (dict(scale=0.9), "scale"), (dict(scale=nan), "scale"), (dict(kernel_depth=2), "kernel_depth"),
                     (dict(kernel_depth=6), "kernel_depth"), (dict(kernel_depth=-1), "kernel_depth"), (dict(samples_per_node=0.0), "samples_per_node"),
                     (dict(samples_per_node=inf), "samples_per_node"), (dict(smooth_steps=-1), "smooth_steps"), (dict(trim=nan), "trim"), (dict(trim=inf), "trim"),
                     (dict(island_ratio=-0.1), "island_ratio"), (dict(island_ratio=1.0), "island_ratio"), (dict(island_ratio=nan), "island_ratio"),
                     (dict(F=bad_i), "index"), (dict(F=neg_i), "index"), (dict(V=bad_c), "finite"), (dict(n_f=(2 ** 31 + 2) // 3), "nf"), (dict(n_f=-1), "nf"),
                     (dict(n_v=-1), "nv"), (dict(n_v=2 ** 31), "nv"), (dict(n=2 ** 31), "INT32_MAX"), (dict(n=-1), "n "), (dict(V=None, n_v=len(v)), "NULL"),
                     (dict(F=None, n_f=len(f)), "NULL"), (dict(S=None, n=3), "NULL"), (dict(pn=None), "NULL")):
        st, msg = call(**kw)
        assert st == RSM_E_INVALID and name in msg and msg.startswith("mesh_trim"), (kw, st, msg)
    assert lib.rsm_mesh_trim(h, ptr(v), C.c_int64(len(v)), ptr(f), C.c_int64(len(f)), ptr(s), None, C.c_int64(3), None, C.byref(nv), C.byref(nf), None) == RSM_E_INVALID
    assert "params" in (lib.rsm_last_error(h) or b"").decode()
    assert call()[0] == 0
    x = np.full(len(v), 8.0)
    for fn in (lambda: ctx.mesh_split(v, bad_i, x), lambda: ctx.mesh_split(bad_c, f, x), lambda: ctx.mesh_split(v, f, np.where(np.arange(len(v)) == 3, np.nan, x)),
               lambda: ctx.mesh_split(v, f, x, island_ratio=1.5), lambda: ctx.mesh_split(v, f, x, trim=np.inf), lambda: ctx.mesh_value_smooth(x, neg_i, 1),
               lambda: ctx.mesh_value_smooth(x, f, -1), lambda: ctx.mesh_value_smooth(np.where(np.arange(len(v)) == 0, np.inf, x), f, 1),
               lambda: ctx.mesh_density(s, None, bad_c, 5), lambda: ctx.mesh_density(s, None, v, 5, kernel_depth=7), lambda: ctx.mesh_trim_last(s, None, depth=3)):
        with pytest.raises(RsmError) as e:
            fn()
        assert e.value.code == RSM_E_INVALID and "mesh_trim" in str(e.value)


def test_empty_meshes_and_no_valid_sample(ctx):
    v, f = mt.plane(5, 5)
    s = np.float32([[0, 0, 0], [4, 4, 1], [2, 1, 0]])
    e3, e3i = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for V, F in ((e3, e3i), (v, e3i)):
        ov, of, st = ctx.mesh_trim(V, F, s, None, depth=5)
        assert ov.shape == (0, 3) and of.shape == (0, 3) and st["n_faces"] == 0 and st["n_valid"] == 3
        assert ctx.poisson_last_mesh(0, 0)[0].shape == (0, 3)
    # no valid sample: every value is 0 -- everything goes at a trim above 0, everything stays at a trim of 0
    nos = np.full((2, 3), np.nan, np.float32)
    ov, of, st = ctx.mesh_trim(v, f, nos, None, depth=5, trim=1.0)
    assert of.shape == (0, 3) and (st["n_valid"], st["n_invalid"], st["value_max"], st["density_step"]) == (0, 2, 0.0, 0.0)
    ov, of, st = ctx.mesh_trim(v, f, nos, None, depth=5, trim=0.0)
    assert ov.tobytes() == v.tobytes() and np.array_equal(of, f) and st["cut_edges"] == 0
    # values all on one side through the stage
    assert ctx.mesh_split(v, f, np.full(len(v), 6.0))[1].shape == (0, 3)
    assert np.array_equal(ctx.mesh_split(v, f, np.full(len(v), 7.0))[1], f)


# ---- 7: API and CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cloud_optimization_run_mesh_trim_then_clean(ctx):
    from reconstruction_amd import Camera, CloudOptimization, ManageData, StereoMatching
    cfgs = [synth.config_small(320, 192, 3, radius=2, pair=4, mask_l0_width=60, border_l0=4),
            synth.config_small(320, 192, 3, radius=2, pair=5, mask_l0_width=50, border_l0=4, holes=True)]
    cam = np.array([0.0, 0.0, 0.0], np.float32)
    top = 1 << (cfgs[0].pyr_levels - 1)
    data = ManageData(cam=[[Camera(camID=0, image=c.image[0], mask=c.mask[0], CamCenter=cam),
                            Camera(camID=1, image=c.image[1], mask=c.mask[1], CamCenter=cam)] for c in cfgs],
                      m_PyrmNum=cfgs[0].pyr_levels, m_LowestLevelSize=(cfgs[0].width // top, cfgs[0].height // top),
                      m_OriginSize=(cfgs[0].width, cfgs[0].height),
                      rectified=[dict(Q=c.Q, R_final=c.R_final, T_final=c.T_final) for c in cfgs])
    opt = CloudOptimization(ctx)
    opt.Init(100, 1, 50, 2, 40.0, data, False)
    sm = StereoMatching(0)
    sm.Init(data, opt, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    sx, sn, _ = opt.run()
    with pytest.raises(ValueError, match="mesh"):
        opt.trim_mesh()
    mv, mf, mst = opt.mesh(depth=7, trim_cells=0)
    vals = ctx.mesh_density(sx, sn, mv, 7)[1]
    t = float(np.median(vals))
    v, f, st = opt.trim_mesh(smooth_steps=5, trim=t)
    assert opt.mesh_result[0] is v and opt.mesh_result[2] is st
    print("run() -> mesh(trim_cells=0) -> trim_mesh(trim=%.3f): %d faces -> %d; %s" % (t, len(mf), len(f), st))
    ev, ef, est = ctx.mesh_trim(mv, mf, sx, sn, depth=7, smooth_steps=5, trim=t)
    assert v.tobytes() == ev.tobytes() and f.tobytes() == ef.tobytes() and st == est
    assert 0 < len(f) < len(mf) + 2 * st["faces_split"] and st["cut_edges"] > 0
    assert (st["n_valid"], st["n_invalid"]) == (mst["n_valid"], mst["n_invalid"]) and st["n_valid"] + st["n_invalid"] == len(sx)   # the Poisson call's samples
    cv, cf, cst = opt.clean_mesh()
    wv, wf, wst = mr.clean(v, f)
    assert cv.tobytes() == wv.tobytes() and np.array_equal(cf, wf) and cst == wst


def test_cli_mesh_density_trim(ctx, tmp_path, capsys):
    from PIL import Image
    from reconstruction_amd import config as cfgmod
    from reconstruction_amd.__main__ import main
    raw = synth.make_raw_pair(baseline=-150.0)
    root = str(tmp_path) + "/"
    (tmp_path / "mask").mkdir()
    for j in range(2):
        Image.fromarray(raw["image"][j][:, :, ::-1]).save(root + "0001_Cam%d.png" % j)
        Image.fromarray(raw["mask"][j]).save(root + "mask/0001_Cam%d.png" % j)
    cfgmod.dump_opencv_yaml(root + "calib_camera.yml", {"intrinsic-0": raw["K"][0], "extrinsic-0": raw["E"][0],
                                                         "intrinsic-1": raw["K"][1], "extrinsic-1": raw["E"][1]})
    cfgmod.dump_opencv_yaml(root + "config.yml", {
        "filepath": root, "outfilename": root + "out", "isoutput": 0, "camera_calib_name": "calib_camera.yml",
        "PyrmNum": raw["pyr_levels"], "LowestLevelWidth": raw["lowest"][0], "LowestLevelHeight": raw["lowest"][1],
        "imagelist": ["0001_Cam%d.png" % j for j in range(2)], "masklist": ["mask\\0001_Cam%d.png" % j for j in range(2)],
        "camID": np.array([[0, 1]], np.uint8)})
    norm = lambda s: re.sub(r"\d+\.\d+ s", "T s", s)
    base = [root + "config.yml", "--mls-radius", "10", "--mesh-depth", "7"]
    capsys.readouterr()
    assert main(base + ["--mesh", "--mesh-trim", "0", "--mesh-out", root + "raw.ply"]) == 0
    plain = norm(capsys.readouterr().out)
    assert "density trim" not in plain
    rv, rf = pr.read_ply_mesh(root + "raw.ply")
    blob = open(root + "bigcloud.ply", "rb").read()
    rec = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], "<f4").reshape(-1, 7)
    sx, sn = rec[:, :3].copy(), rec[:, 3:].copy()
    t = float(np.median(ctx.mesh_density(sx, sn, rv, 7)[1]))
    assert main(base + ["--mesh-density-trim", repr(t), "--mesh-density-smooth", "3", "--mesh-trim", "2"]) == 0      # implies --mesh; --mesh-trim is not applied
    out = norm(capsys.readouterr().out)
    v, f = pr.read_ply_mesh(root + "bigmesh.ply")
    ev, ef, est = ctx.mesh_trim(rv, rf, sx, sn, depth=7, smooth_steps=3, trim=t)
    assert v.tobytes() == ev.tobytes() and np.array_equal(f, ef) and 0 < len(f)
    lines = out.splitlines()
    assert lines[:-2] == plain.splitlines()[:-1] and lines[-2].startswith("Mesh density trim: %d faces from %d" % (est["n_faces"], est["n_faces_in"]))
    assert lines[-1] == "%d vertices, %d faces -> %sbigmesh.ply" % (len(v), len(f), root)
    # given bare, T is mesh.bat's 7; the island ratio reaches the library
    assert main(base + ["--mesh-island-ratio", "0", "--mesh-out", root + "m7.ply", "--mesh-density-trim"]) == 0
    e7 = ctx.mesh_trim(rv, rf, sx, sn, depth=7, island_ratio=0.0)[2]
    assert "Mesh density trim: %d faces from %d" % (e7["n_faces"], e7["n_faces_in"]) in capsys.readouterr().out
    assert main(base + ["--mesh-density-trim", "--mesh-island-ratio", "1.5"]) == 1
    assert "island_ratio" in capsys.readouterr().out
