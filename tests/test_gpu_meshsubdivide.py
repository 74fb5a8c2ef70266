"""GPU Loop subdivision (csrc/k_meshsubdivide.hip) against the numpy restatement (tests/meshsubdivide_restatement.py):
split flags, odd and even positions, vertex classes, faces and stats are the restatement's exactly -- the same faces in the same order, the
same bits.  Integers apart, everything is fp64 + - * in a fixed order with beta_k from the host's libm, and integer atomics.  If bits differ,
look for a contracted multiply-add or another order of a sum; the comparison is not to be loosened.

Meshes of more than ~1000 faces run one iteration (the restatement is Python loops); three iterations run on the small solids only.  The
refusal of a result that would be too large is held by tests/cpp/subdivide_limits_check.cpp (tests/test_meshsubdivide_cpu.py): reaching it
on a GPU takes 1.8e8 faces."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mesh_topology_fixtures as mt
import meshclose_restatement as mc
import meshsubdivide_restatement as ms
import poisson_restatement as pr
from reconstruction_amd import synth

pytestmark = pytest.mark.gpu

NF_BIG = (2 ** 31 + 2) // 3


def _random_vertices(nv, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (nv, 3)).astype(np.float32)


STAGE_MESHES = {
    "tetrahedron": ms.tetrahedron, "octahedron": ms.octahedron, "icosahedron": ms.icosahedron, "lattice": ms.lattice,
    "plane_5x5": lambda: mc.plane(5, 5), "cut_plane": mc.cut_plane, "annulus_16": lambda: mc.annulus(16), "bow_tie": ms.bow_tie,
    "against": lambda: (_random_vertices(4, 1), np.int32([[0, 1, 2], [0, 1, 3]])), "alike": lambda: (_random_vertices(4, 2), np.int32([[0, 1, 2], [1, 0, 3]])),
    "three_face_edge": ms.three_face_edge, "repeated_index": lambda: (_random_vertices(5, 3), np.int32([[0, 1, 1], [2, 3, 4], [4, 4, 4]])),
    "square_patch": ms.square_patch, "patterns": ms.pattern_mesh,
}


def same_stage(ctx, v, f, **kw):
    got = ctx.mesh_subdivide_edges(v, f, **kw)
    want = ms.loop_step(v, f, ms.threshold_of(v, kw.get("threshold", 0.0), kw.get("threshold_fraction", 0.0)))
    assert got["threshold"] == ms.threshold_of(v, kw.get("threshold", 0.0), kw.get("threshold_fraction", 0.0))
    for k in ("keys", "multiplicity", "split", "odd", "vertex_class", "even"):
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (k, np.nonzero(np.atleast_1d((g != w).reshape(len(g), -1).any(1)))[0][:8])
    return got, want


def same_whole(ctx, v, f, **kw):
    """the whole call on a host mesh against the restatement: (vertices, faces, stats)"""
    wv, wf, wst = ms.subdivide(v, f, **kw)
    ov, of, st = ctx.mesh_subdivide(v, f, **kw)
    assert ov.dtype == np.float32 and of.dtype == np.int32
    assert of.shape == wf.shape and of.tobytes() == wf.tobytes()
    assert ov.shape == wv.shape and ov.tobytes() == wv.tobytes()
    assert st == wst, {k: (st[k], wst[k]) for k in st if st[k] != wst[k]}
    return ov, of, st


# ---- 1: the stage entry ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STAGE_MESHES))
def test_stage_decisions_are_the_restatements_bits(ctx, name):
    v, f = STAGE_MESHES[name]()
    got, want = same_stage(ctx, v, f)                                  # thr = 0: every edge splits
    assert got["split"].all() or len(got["split"]) == 0
    l2 = np.sort([ms.len2(v[int(k) >> 32].astype(np.float64), v[int(k) & 0xFFFFFFFF].astype(np.float64)) for k in got["keys"]])
    thr = math.sqrt(float(l2[len(l2) // 2]))                           # about the median length: the edges with l2 > thr thr split, as the rule says
    got, want = same_stage(ctx, v, f, threshold=thr)
    assert int(got["split"].sum()) == int((l2 > thr * thr).sum())
    same_stage(ctx, v, f, threshold_fraction=0.25)
    if name == "bow_tie":
        assert got["vertex_class"].tolist() == [1, 1, 2, 1, 1]
    if name == "three_face_edge":
        assert got["multiplicity"].max() == 3 and got["vertex_class"][:2].tolist() == [2, 2]
    if name == "icosahedron":
        assert (got["vertex_class"] == 0).all() and (got["multiplicity"] == 2).all()


def test_stage_on_empty_meshes(ctx):
    e3, e3i = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    v = _random_vertices(7, 4)
    got = ctx.mesh_subdivide_edges(e3, e3i)
    assert len(got["keys"]) == 0 and len(got["even"]) == 0
    got, want = same_stage(ctx, v, e3i, threshold_fraction=0.5)
    assert (got["vertex_class"] == 2).all() and got["even"].tobytes() == v.tobytes()


# ---- 2: whole calls at thr = 0 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tetrahedron", "octahedron", "icosahedron"])
def test_three_iterations_are_three_calls_of_one(ctx, name):
    v, f = STAGE_MESHES[name]()
    ov, of, st = same_whole(ctx, v, f, iterations=3)
    assert st["iterations"] == 3 and len(of) == 64 * len(f) and st["faces_3_splits"] == 21 * len(f)
    sv, sf = v, f
    for _ in range(3):
        sv, sf, st1 = ctx.mesh_subdivide(sv, sf, iterations=1)
        assert st1["iterations"] == 1
    assert sv.tobytes() == ov.tobytes() and sf.tobytes() == of.tobytes()
    ov2, of2, st2 = ctx.mesh_subdivide(v, f, iterations=3)            # the second call on the same input
    assert ov2.tobytes() == ov.tobytes() and of2.tobytes() == of.tobytes() and st2 == st


def _grey_views():
    from reconstruction_amd import Camera
    P = np.array([[20.0, 0, 0, 0], [0, 20.0, 0, 0], [0, 0, 1.0, 40.0]])
    img = np.full((64, 64, 3), 90, np.uint8)
    return [[Camera(camID=0, image=img, mask=None, P=P), Camera(camID=1, image=img, mask=None, P=P)]]


def _last_colors(ctx, nv):
    rgb = np.zeros((max(nv, 1), 3), np.uint8)
    return ctx._lib.rsm_mesh_last_colors(ctx._h, rgb.ctypes.data_as(C.c_void_p), None)


def test_three_entries_the_last_mesh_and_its_colours(ctx):
    from reconstruction_amd import RsmError
    from reconstruction_amd._lib import RSM_E_INVALID, RSM_E_STATE
    v, f = ms.icosahedron()
    wv, wf, wst = ms.subdivide(v, f, iterations=2)
    ov, of, st = ctx.mesh_subdivide(v, f, iterations=2)
    hv, hf = ctx.poisson_last_mesh(len(ov), len(of))
    assert hv.tobytes() == ov.tobytes() == wv.tobytes() and hf.tobytes() == of.tobytes() == wf.tobytes() and st == wst
    dv, df = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    nv, nf, st2 = ctx.mesh_subdivide_device(dv.data_ptr(), len(v), df.data_ptr(), len(f), iterations=2)
    assert (nv, nf) == (len(wv), len(wf)) and st2 == st
    o_v, o_f = torch.empty((nv, 3), dtype=torch.float32, device="cuda"), torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    ctx.poisson_last_mesh_device(o_v.data_ptr(), o_f.data_ptr())
    assert o_v.cpu().numpy().tobytes() == wv.tobytes() and o_f.cpu().numpy().tobytes() == wf.tobytes()
    assert torch.equal(dv.cpu(), torch.from_numpy(v)) and torch.equal(df.cpu(), torch.from_numpy(f))      # the input is not written
    # colours set on the last mesh; a refused call leaves them and the mesh, a call that is taken drops them
    assert len(ctx.mesh_color_last(_grey_views(), 0.5)[0]) == nv and _last_colors(ctx, nv) == 0
    for bad in (dict(iterations=0), dict(weight_scheme=2), dict(threshold=-1.0)):
        with pytest.raises(RsmError) as e:
            ctx.mesh_subdivide_last(**bad)
        assert e.value.code == RSM_E_INVALID
        assert _last_colors(ctx, nv) == 0
    hv, hf = ctx.poisson_last_mesh(nv, nf)
    assert hv.tobytes() == wv.tobytes() and hf.tobytes() == wf.tobytes()
    lv, lf, lst = ctx.mesh_subdivide_last(iterations=1)
    w2 = ms.subdivide(wv, wf, iterations=1)
    assert lv.tobytes() == w2[0].tobytes() and lf.tobytes() == w2[1].tobytes() and lst == w2[2]
    assert _last_colors(ctx, len(lv)) == RSM_E_STATE
    hv, hf = ctx.poisson_last_mesh(len(lv), len(lf))
    assert hv.tobytes() == lv.tobytes() and hf.tobytes() == lf.tobytes()
    assert len(ctx.mesh_color_last(_grey_views(), 0.5)[0]) == len(lv)  # the subdivided mesh is coloured like any other
    # ... and a call that splits nothing still replaces the mesh (by its copy) and drops the colours, as every stage that is taken does
    nv3, nf3, st3 = ctx.mesh_subdivide_device(dv.data_ptr(), len(v), df.data_ptr(), len(f), threshold=100.0)
    assert (nv3, nf3, st3["iterations"]) == (len(v), len(f), 0) and _last_colors(ctx, nv3) == RSM_E_STATE


def test_empty_meshes(ctx):
    from reconstruction_amd import Context
    e3, e3i = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    ov, of, st = same_whole(ctx, e3, e3i)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and st["iterations"] == 0
    v = _random_vertices(9, 5)
    ov, of, st = same_whole(ctx, v, e3i, threshold_fraction=0.01)      # vertices without a face stay
    assert ov.tobytes() == v.tobytes() and of.shape == (0, 3)
    fresh = Context(0)                                                 # a context without a mesh: an empty mesh and RSM_OK
    ov, of, st = fresh.mesh_subdivide_last()
    assert ov.shape == (0, 3) and of.shape == (0, 3) and st["n_vertices_in"] == 0
    fresh.close()


# ---- 3: adaptive ----------------------------------------------------------------------------------------------------------------------------------
def test_an_edge_exactly_at_the_threshold_stays(ctx):
    v, f = np.float32([[0, 0, 0], [3, 0, 0], [3, 4, 0]]), np.int32([[0, 1, 2]])       # edges 3, 4 and 5, exactly
    ov, of, st = same_whole(ctx, v, f, iterations=1, threshold=5.0)
    assert st["iterations"] == 0 and ov.tobytes() == v.tobytes() and of.tobytes() == f.tobytes()
    below = math.nextafter(5.0, 0.0)
    ov, of, st = same_whole(ctx, v, f, iterations=1, threshold=below)
    assert st["iterations"] == 1 and st["split_edges"] == 1 and st["faces_1_split"] == 1 and len(of) == 2
    ov, of, st = same_whole(ctx, v, f, iterations=1, threshold=4.0)
    assert st["split_edges"] == 1
    ov, of, st = same_whole(ctx, v, f, iterations=1, threshold=math.nextafter(4.0, 0.0))
    assert st["split_edges"] == 2 and st["faces_2_splits"] == 1 and len(of) == 3


def test_every_pattern_and_both_diagonals(ctx):
    v, f = ms.pattern_mesh()
    ov, of, st = same_whole(ctx, v, f, iterations=1, threshold=ms.PATTERN_THR)
    assert [st["faces_0_splits"], st["faces_1_split"], st["faces_2_splits"], st["faces_3_splits"]] == ms.PATTERN_COUNTS
    assert ms.loop_step(v, f, ms.PATTERN_THR)["diagonals"] == ms.PATTERN_DIAGONALS
    same_whole(ctx, v, f, iterations=3, threshold=ms.PATTERN_THR)      # later iterations split what is still long, then stop
    v, f = mt.grid()                                                   # a connected mesh: jittered cells, their diagonals longer than their sides
    ov, of, st = same_whole(ctx, v, f, iterations=1, threshold=1.1)
    assert min(st["faces_1_split"], st["faces_2_splits"], st["faces_3_splits"]) > 0
    same_whole(ctx, v, f, iterations=3, threshold=0.6)


def test_fraction_is_the_absolute_threshold_of_the_box(ctx):
    v, f = mt.grid()
    ov, of, st = same_whole(ctx, v, f, iterations=1, threshold_fraction=0.07)
    thr = 0.07 * ms.box_diagonal(v)
    assert st["threshold"] == thr and 0 < st["split_edges"] < len(ms.edge_runs(f))
    av, af, ast = ctx.mesh_subdivide(v, f, iterations=1, threshold=thr)
    assert av.tobytes() == ov.tobytes() and af.tobytes() == of.tobytes() and ast == st
    fv, ff, fst = ctx.mesh_subdivide(v, f, iterations=1, threshold=1e9, threshold_fraction=0.07)      # the fraction wins
    assert ff.tobytes() == of.tobytes() and fst == st
    sv, sf, sst = same_whole(ctx, v, f, threshold_fraction=1.0)        # nothing is longer than the diagonal: the input's bytes
    assert sst["iterations"] == 0 and sv.tobytes() == v.tobytes() and sf.tobytes() == f.tobytes() and sst["split_edges"] == 0


# ---- 4: unfriendly topology, one iteration each ------------------------------------------------------------------------------------------------------
TOPOLOGY = (["hub_%d" % n for n in (63, 64, 65, 255, 256, 257, 1000)] + ["hub_%d_closed" % n for n in (63, 64, 65, 255, 256, 257)] +
            ["book_%d" % n for n in (63, 64, 65, 255, 256, 257, 1000)] + ["book_65_dup", "book_257_dup"] + mt.names("book_in_grid", "strip_", "pieces", "padded_"))


def _topology_mesh(name):
    if name in mt.CATALOGUE:
        return mt.get(name)
    assert name.startswith("book_")
    return mt.book(int(name.split("_")[1]))


@pytest.mark.parametrize("name", TOPOLOGY)
def test_unfriendly_topology_one_iteration(ctx, name):
    v, f = _topology_mesh(name)
    ov, of, st = same_whole(ctx, v, f, iterations=1)
    assert st["iterations"] == 1 and 0 < st["split_edges"] <= len(ms.edge_runs(f))
    if name.startswith("hub_1000"):
        assert st["max_valence"] == 1000 and st["moved_interior"] == 1
    if name.startswith("book_1000"):
        assert st["split_many_face_edges"] == 1 and st["max_valence"] == 1000
    # ... and with the median edge length as the threshold: that edge stays with the shorter half, the longer half splits
    P = v.astype(np.float64)
    lengths = np.sort([math.sqrt(ms.len2(P[a], P[b])) for (a, b), _ in ms.edge_runs(f)])
    ov, of, st = same_whole(ctx, v, f, iterations=1, threshold=float(lengths[len(lengths) // 2]))
    print("%s: %s" % (name, st))
    assert 0 < st["split_edges"] < len(lengths)


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------------------------
TEXTS = {
    "params": "mesh_subdivide: params is NULL",
    "null": "mesh_subdivide: a NULL pointer",
    "nv": "mesh_subdivide: nv -1 outside 0..INT32_MAX",
    "nf": "mesh_subdivide: nf 715827883 negative or 3 nf >= 2^31",
    "index": "mesh_subdivide: a face index outside [0, nv)",
    "finite": "mesh_subdivide: a coordinate that is not finite",
}
CASES = (
    (dict(params=None), "params", ("host", "device", "last")),
    (dict(pn=None), "null", ("host", "device", "last")),
    (dict(V=None), "null", ("host", "device")),
    (dict(n_v=-1), "nv", ("host", "device")),
    (dict(n_f=NF_BIG), "nf", ("host", "device")),
    (dict(F="bad_index"), "index", ("host", "device")),
    (dict(V="nan"), "finite", ("host", "device")),
    (dict(params=None, n_v=-1), "params", ("host", "device")),
    (dict(n_v=-1, pn=None), "nv", ("host", "device")),
)
OWN = (
    (dict(iterations=0), "mesh_subdivide: iterations 0 outside 1..8"),
    (dict(iterations=9), "mesh_subdivide: iterations 9 outside 1..8"),
    (dict(threshold=-1.0), "mesh_subdivide: threshold -1 negative or not finite"),
    (dict(threshold=float("inf")), "mesh_subdivide: threshold inf negative or not finite"),
    (dict(threshold=float("nan")), "mesh_subdivide: threshold nan negative or not finite"),
    (dict(threshold_fraction=-0.5), "mesh_subdivide: threshold_fraction -0.5 outside [0, 1]"),
    (dict(threshold_fraction=1.5), "mesh_subdivide: threshold_fraction 1.5 outside [0, 1]"),
    (dict(threshold_fraction=float("nan")), "mesh_subdivide: threshold_fraction nan outside [0, 1]"),
    (dict(weight_scheme=1), "mesh_subdivide: weight_scheme 1 not 0"),
    (dict(weight_scheme=2), "mesh_subdivide: weight_scheme 2 not 0"),
    (dict(weight_scheme=-1), "mesh_subdivide: weight_scheme -1 not 0"),
)


@pytest.fixture(scope="module")
def meshes():
    v, f = mc.plane(5, 5)
    v = v.copy()
    v[:, 2] = np.random.default_rng(8).uniform(-0.2, 0.2, len(v)).astype(np.float32)
    assert v.shape == (25, 3) and f.shape == (32, 3)
    bad_i, bad_c = f.copy(), v.copy()
    bad_i[7, 1] = len(v)
    bad_c[3, 2] = np.nan
    host = {"V": v, "F": f, "bad_index": bad_i, "nan": bad_c}
    dev = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
    return host, dev


def _call(ctx, meshes, entry, V="V", F="F", n_v=None, n_f=None, pn="given", params="given", **kw):
    lib, h = ctx._lib, ctx._h
    host, dev = meshes
    nv, nf = C.c_int64(), C.c_int64()
    prm = ctx.mesh_subdivide_params(**dict(dict(iterations=1), **kw))
    p = C.byref(prm) if params is not None else None
    if entry == "host":
        ptr = lambda k: None if k is None else host[k].ctypes.data_as(C.c_void_p)
    else:
        ptr = lambda k: None if k is None else C.c_void_p(dev[k].data_ptr())
    mesh = () if entry == "last" else (ptr(V), C.c_int64(25 if n_v is None else n_v), ptr(F), C.c_int64(32 if n_f is None else n_f))
    fn = getattr(lib, "rsm_mesh_subdivide%s" % {"host": "", "device": "_device", "last": "_last"}[entry])
    st = fn(h, *mesh, p, C.byref(nv) if pn is not None else None, C.byref(nf), None)
    return st, (lib.rsm_last_error(h) or b"").decode()


def test_refusals_say_the_house_texts_and_the_stages_own(ctx, meshes):
    from reconstruction_amd import RsmError
    from reconstruction_amd._lib import RSM_E_INVALID
    for entry in ("host", "device", "last"):
        if entry == "last":
            ctx.mesh_subdivide(meshes[0]["V"], meshes[0]["F"], threshold=100.0)      # a small last mesh for the calls that are taken
        assert _call(ctx, meshes, entry)[0] == 0, entry
        for spoil, name, entries in CASES:
            if entry in entries:
                st, msg = _call(ctx, meshes, entry, **spoil)
                assert (st, msg) == (RSM_E_INVALID, TEXTS[name]), (entry, spoil, st, msg)
        for spoil, text in OWN:
            st, msg = _call(ctx, meshes, entry, **spoil)
            assert st == RSM_E_INVALID and msg.startswith(text), (entry, spoil, st, msg)
        assert _call(ctx, meshes, entry, iterations=8, threshold=50.0)[0] == 0 and _call(ctx, meshes, entry, threshold_fraction=1.0)[0] == 0
    v, f = meshes[0]["V"], meshes[0]["F"]
    for fn in (lambda: ctx.mesh_subdivide(v, f, iterations=9), lambda: ctx.mesh_subdivide_edges(v, meshes[0]["bad_index"]),
               lambda: ctx.mesh_subdivide_edges(meshes[0]["nan"], f), lambda: ctx.mesh_subdivide_edges(v, f, weight_scheme=2),
               lambda: ctx.mesh_subdivide_device(0, len(v), 0, len(f))):
        with pytest.raises(RsmError) as e:
            fn()
        assert e.value.code == RSM_E_INVALID and "mesh_subdivide" in str(e.value)


# ---- 6: CLI ---------------------------------------------------------------------------------------------------------------------------------------
def test_cli_mesh_subdivide(ctx, tmp_path, capsys):
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
    base = [root + "config.yml", "--mls-radius", "10", "--mesh-depth", "5"]        # (depth 5: the restatement runs on this mesh as well)
    capsys.readouterr()
    assert main(base + ["--mesh-clean", "--mesh-decimate", "400", "--mesh-out", root + "coarse.ply"]) == 0
    assert "Mesh subdivide" not in capsys.readouterr().out
    cv, cf = pr.read_ply_mesh(root + "coarse.ply")
    assert 300 < len(cf) <= 400
    # the flag implies --mesh, runs after --mesh-decimate and before the colouring; 2 iterations at 2 % of the box diagonal
    assert main(base + ["--mesh-clean", "--mesh-decimate", "400", "--mesh-subdivide", "2", "--mesh-subdivide-threshold", "2", "--mesh-color"]) == 0
    out = capsys.readouterr().out
    v, f = pr.read_ply_mesh(root + "bigmesh.ply")
    wv, wf, wst = ms.subdivide(cv, cf, iterations=2, threshold_fraction=2 / 100.0)
    assert len(f) == len(wf) > 4 * len(cf) and v.tobytes() == wv.tobytes() and np.array_equal(f, wf)
    line = [l for l in out.splitlines() if l.startswith("Mesh subdivide:")]
    assert len(line) == 1 and line[0].startswith("Mesh subdivide: %d -> %d faces, %d -> %d vertices in %d iterations (threshold %.6g); %d edges split"
                                                 % (len(cf), len(wf), len(cv), len(wv), wst["iterations"], wst["threshold"], wst["split_edges"]))
    lines = out.splitlines()
    written = "%d vertices, %d faces -> %sbigmesh.ply" % (len(v), len(f), root)
    assert written in lines and lines.index([l for l in lines if l.startswith("Mesh decimate:")][0]) < lines.index(line[0]) < lines.index(written)
    colour = [l for l in lines if l.startswith("Mesh colour:")]
    assert len(colour) == 1 and " of %d vertices coloured" % len(v) in colour[0]      # the colouring ran on the subdivided mesh
