"""What the four mesh-to-mesh stages (clean, trim, close_holes, decimate) say when they refuse a call, through each of their entries (host,
_device, _last), and who owns the colours of the context's last mesh (csrc/rsm_mesh.hip).  The entries share one host path; the texts below
are written out as the library has always said them, status and whole string, and two double faults per stage pin the order of the checks:
params, counts, the stage's own (trim's n), pointers, then the mesh itself on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import meshdecimate_restatement as md
import poisson_restatement as pr

pytestmark = pytest.mark.gpu

NF_BIG = (2 ** 31 + 2) // 3          # 715827883: the least nf with 3 nf >= 2^31

TEXTS = {
    "clean": {
        "params": "mesh_clean: params is NULL",
        "null": "mesh_clean: a NULL pointer",
        "nv": "mesh_clean: nv -1 outside 0..INT32_MAX",
        "nf": "mesh_clean: nf 715827883 negative or 3 nf >= 2^31",
        "index": "mesh_clean: a face index outside [0, nv)",
        "finite": "mesh_clean: a coordinate that is not finite",
    },
    "trim": {
        "params": "mesh_trim: params is NULL",
        "null": "mesh_trim: a NULL pointer",
        "nv": "mesh_trim: nv -1 outside 0..INT32_MAX",
        "nf": "mesh_trim: nf 715827883 negative or 3 nf >= 2^31",
        "index": "mesh_trim: a face index outside [0, nv)",
        "finite": "mesh_trim: a coordinate that is not finite",
        "n": "mesh_trim: n -1 outside 0..INT32_MAX",
    },
    "close_holes": {
        "params": "mesh_close_holes: params is NULL",
        "null": "mesh_close_holes: a NULL pointer",
        "nv": "mesh_close_holes: nv -1 outside 0..INT32_MAX",
        "nf": "mesh_close_holes: nf 715827883 negative or 3 nf >= 2^31",
        "index": "mesh_close_holes: a face index outside [0, nv)",
        "finite": "mesh_close_holes: a coordinate that is not finite",
    },
    "decimate": {
        "params": "mesh_decimate: params is NULL",
        "null": "mesh_decimate: a NULL pointer",
        "nv": "mesh_decimate: nv -1 outside 0..INT32_MAX",
        "nf": "mesh_decimate: nf 715827883 negative or 3 nf >= 2^31",
        "index": "mesh_decimate: a face index outside [0, nv)",
        "finite": "mesh_decimate: a coordinate that is not finite",
    },
}

# (what is wrong, the text it must name, the entries it applies to); the last two are the double faults
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


def _params(ctx, stage):
    from reconstruction_amd._lib import MeshCloseParams, MeshTrimParams
    if stage == "clean":
        return ctx._mesh_clean_params(0, True, True, 0.0, False, True, True, True)
    if stage == "trim":
        return MeshTrimParams(5, 1.1, 0, 1.0, 0, 0.0, 0.0)
    if stage == "close_holes":
        return MeshCloseParams(30)
    return ctx.mesh_decimate_params(target_faces=10)


@pytest.fixture(scope="module")
def meshes():
    """the small mesh and its two spoilt copies, on the host and on the device"""
    v, f = md.grid_mesh(5)
    assert v.shape == (25, 3) and f.shape == (32, 3)
    bad_i, bad_c = f.copy(), v.copy()
    bad_i[7, 1] = len(v)
    bad_c[3, 2] = np.nan
    host = {"V": v, "F": f, "bad_index": bad_i, "nan": bad_c}
    dev = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
    return host, dev


def _call(ctx, meshes, stage, entry, V="V", F="F", n_v=None, n_f=None, pn="given", n=None, **kw):
    """one call of rsm_mesh_<stage><entry> with what the case spoils -> (status, rsm_last_error)"""
    lib, h = ctx._lib, ctx._h
    host, dev = meshes
    nv, nf = C.c_int64(), C.c_int64()
    prm = _params(ctx, stage)
    p = C.byref(prm) if kw.get("params", prm) is not None else None
    if entry == "host":
        ptr = lambda k: None if k is None else host[k].ctypes.data_as(C.c_void_p)
    else:
        ptr = lambda k: None if k is None else C.c_void_p(dev[k].data_ptr())
    mesh = () if entry == "last" else (ptr(V), C.c_int64(25 if n_v is None else n_v), ptr(F), C.c_int64(32 if n_f is None else n_f))
    # (trim's samples: the vertices, no normals; only the _device entry takes them on the device)
    sx = C.c_void_p(dev["V"].data_ptr()) if entry == "device" else host["V"].ctypes.data_as(C.c_void_p)
    samples = (sx, None, C.c_int64(25 if n is None else n)) if stage == "trim" else ()
    fn = getattr(lib, "rsm_mesh_%s%s" % (stage, {"host": "", "device": "_device", "last": "_last"}[entry]))
    st = fn(h, *mesh, *samples, p, C.byref(nv) if pn is not None else None, C.byref(nf), None)
    return st, (lib.rsm_last_error(h) or b"").decode()


@pytest.mark.parametrize("stage", ("clean", "trim", "close_holes", "decimate"))
def test_refusals_say_what_they_always_said(ctx, meshes, stage):
    from reconstruction_amd._lib import RSM_E_INVALID
    for entry in ("host", "device", "last"):
        assert _call(ctx, meshes, stage, entry)[0] == 0, (stage, entry)            # the unspoilt call is taken
        for spoil, name, entries in CASES:
            if entry in entries:
                st, msg = _call(ctx, meshes, stage, entry, **spoil)
                assert (st, msg) == (RSM_E_INVALID, TEXTS[stage][name]), (stage, entry, spoil, st, msg)
    if stage == "trim":
        for entry in ("host", "device", "last"):
            st, msg = _call(ctx, meshes, stage, entry, n=-1)
            assert (st, msg) == (RSM_E_INVALID, TEXTS["trim"]["n"]), (entry, st, msg)


def _grey_views():
    from reconstruction_amd import Camera
    P = np.array([[20.0, 0, 0, 0], [0, 20.0, 0, 0], [0, 0, 1.0, 40.0]])
    img = np.full((64, 64, 3), 90, np.uint8)
    return [[Camera(camID=0, image=img, mask=None, P=P), Camera(camID=1, image=img, mask=None, P=P)]]


def _last_colors(ctx, nv):
    rgb = np.zeros((max(nv, 1), 3), np.uint8)
    return ctx._lib.rsm_mesh_last_colors(ctx._h, rgb.ctypes.data_as(C.c_void_p), None)


def test_colours_follow_the_mesh_through_mesh_clean(ctx, meshes):
    """A clean that removes nothing leaves a mesh of the same nv, and the allocator may hand it the address the coloured mesh had: the colours
    are still those of the mesh that went."""
    from reconstruction_amd._lib import RSM_E_STATE
    v, f = meshes[0]["V"], meshes[0]["F"]
    ov, of, _ = ctx.mesh_clean(v, f, smooth_steps=0, min_piece=0)
    assert len(ov) == 25 and len(of) == 32
    assert len(ctx.mesh_color_last(_grey_views(), 0.5)[0]) == 25 and _last_colors(ctx, 25) == 0
    for _ in range(2):
        lv, lf, _st = ctx.mesh_clean_last(smooth_steps=0, min_piece=0)
        assert len(lv) == 25 and len(lf) == 32
        assert _last_colors(ctx, 25) == RSM_E_STATE


def test_colours_follow_the_mesh_through_poisson_mesh(ctx):
    from reconstruction_amd._lib import RSM_E_STATE
    xyz, nrm = pr.sphere_samples(2000)
    pv, pf, _ = ctx.poisson_mesh(xyz, nrm, 5)
    assert len(pv) > 0 and len(ctx.mesh_color_last(_grey_views(), 0.5)[0]) == len(pv) and _last_colors(ctx, len(pv)) == 0
    qv, qf, _ = ctx.poisson_mesh(xyz, nrm, 5)
    assert len(qv) == len(pv) and len(qf) == len(pf)
    assert _last_colors(ctx, len(qv)) == RSM_E_STATE
