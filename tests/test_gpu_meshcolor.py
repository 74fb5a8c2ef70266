"""GPU mesh colouring (csrc/k_meshcolor.hip) against the numpy restatement (tests/meshcolor_restatement.py, itself tested
in tests/test_meshcolor_cpu.py) and against answers worked out analytically.  Everything is exact: colours, best views, counts and the depth
buffers' bits are equal -- every operation is an IEEE basic operation in a fixed order and the buffer is an integer maximum.  If bits
differ, look for a contracted multiply-add or another order of summation; the comparison is not to be loosened."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import meshcolor_restatement as mr
import poisson_restatement as pr
from reconstruction_amd import Camera, synth

pytestmark = pytest.mark.gpu

EYE_P = np.hstack([np.eye(3), np.zeros((3, 1))])
K96 = np.array([[50.0, 0, 48.0], [0, 50.0, 36.0], [0, 0, 1.0]])
GREY = [127, 127, 127]
_cache = {}


def sphere(ctx):
    """the GPU's own depth-5 Poisson mesh of the sphere samples (radius 50 round (10, -20, 600)), about 6 k faces: (vertices, faces, h)"""
    if "sphere" not in _cache:
        xyz, nrm = pr.sphere_samples(20000)
        v, f, st = ctx.poisson_mesh(xyz, nrm, 5, trim_cells=0)
        _cache["sphere"] = (v, f, st["h"])
    return _cache["sphere"]


def cam_pair(P0, img0, m0, P1, img1, m1):
    return [Camera(camID=0, P=P0, image=img0, mask=m0), Camera(camID=1, P=P1, image=img1, mask=m1)]


def sphere_camera(azimuth_deg, elevation_deg=0.0, dist=250.0, fx=150.0, W=96, H=72):
    a, e = np.radians(azimuth_deg), np.radians(elevation_deg)
    eye = pr.SPHERE_C + dist * np.array([np.sin(a) * np.cos(e), np.sin(e), -np.cos(a) * np.cos(e)])
    return mr.look_at(eye, pr.SPHERE_C, fx, W / 2.0, H / 2.0), eye


def random_image(seed, W, H):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


# ---- 1: texture_color ---------------------------------------------------------------------------------------------------------------------
def test_texture_color_is_the_restatements_bytes(ctx):
    W, H = 64, 48
    P, eye = sphere_camera(25.0, 10.0, fx=90.0, W=W, H=H)
    img = random_image(11, W, H)
    rng = np.random.default_rng(12)
    M, C0 = P[:, :3], mr.cam_center(P)

    def back(u, v, s):                                       # the point at depth s on the ray of pixel (u, v)
        u, v, s = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(s, np.float64))
        return C0 + (np.linalg.solve(M, np.stack([u, v, np.ones_like(u)])) * s).T

    pts = [back(rng.uniform(-10, W + 10, 5000), rng.uniform(-10, H + 10, 5000), rng.uniform(100, 400, 5000))]
    d = np.array([-0.02, -0.001, 0.001, 0.02])
    for e in (-0.5, W - 0.5):                                # just outside / inside the left and right border ...
        pts.append(back(e + d, 20.0, 250.0))
    for e in (-0.5, H - 0.5):                                # ... and the top and bottom one
        pts.append(back(30.0, e + d, 250.0))
    pts.append(back([-0.7, -1.2, -1.49, -0.51, 5.0, 7.0], [5.0, 7.0, 9.0, -0.7, -1.2, -1.49], 250.0))   # quotients in (-1.5, -0.5): pixel 0
    pts.append(back([10.0, 20.0, 30.0], [10.0, 20.0, 30.0], 0.0))                                       # q2 = 0 (up to rounding)
    pts.append(back([10.0, 20.0, 63.0], [10.0, 40.0, 47.0], -250.0))                                    # behind the camera: coloured all the same
    pts.append(np.array([[np.nan, 0, 0], [0, np.inf, 600.0], [1e30, 1e30, 1e30]]))
    xyz = np.concatenate(pts).astype(np.float32)
    exact = np.float32([[-0.7, 3.0, 1.0], [2.0, -1.4, 1.0], [-1.5, 0.0, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [-3.0, -2.0, -1.0]])
    got = ctx.texture_color(xyz, P, img)
    want = mr.texture_color(xyz, P, img)
    grey = (want == 127).all(axis=1)
    print("texture_color: %d points, %d grey" % (len(xyz), grey.sum()))
    assert got.tobytes() == want.tobytes()
    assert 500 < grey.sum() < 4000 and not grey[-6:-3].all()
    # the identity camera: answers by hand (tests/test_meshcolor_cpu.py), quotient -0.7 on pixel 0 and the BGR -> RGB swap
    got = ctx.texture_color(exact, EYE_P, img)
    assert got.tobytes() == mr.texture_color(exact, EYE_P, img).tobytes()
    assert got.tolist() == [img[3, 0, ::-1].tolist(), img[0, 2, ::-1].tolist(), GREY, GREY, GREY, img[2, 3, ::-1].tolist()]
    assert ctx.texture_color(np.zeros((0, 3)), P, img).shape == (0, 3)


# ---- 2: the depth buffer ------------------------------------------------------------------------------------------------------------------
def check_depth(ctx, v, f, P, W, H, label):
    got = ctx.mesh_depth(v, f, P, W, H)
    want = mr.depth_buffer(v, f, P, W, H)
    print("%s: %d of %d pixels drawn, pixels whose bits differ: %d" % (label, (want != 0).sum(), W * H, (got != want).sum()))
    assert got.tobytes() == want.tobytes()
    return got


def big_scene():
    """one triangle covering the whole 96 x 72 image at depth 10 (a box of 6 912 pixels), behind several small ones"""
    rng = np.random.default_rng(21)
    v = [[-1000.0, -1000.0, 10.0], [4000.0, -1000.0, 10.0], [-1000.0, 4000.0, 10.0]]
    f = [[0, 1, 2]]
    for _ in range(12):
        c = np.array([rng.uniform(5, 90), rng.uniform(5, 65)])
        z = rng.uniform(3.0, 8.0, 3)
        for k in range(3):
            p = c + rng.uniform(-6, 6, 2)
            v.append([p[0] * z[k], p[1] * z[k], z[k]])
        f.append([len(v) - 3, len(v) - 2, len(v) - 1])
    return np.float32(v), np.int32(f)


def test_depth_buffer_of_the_sphere_is_the_restatements_bits(ctx):
    v, f, _ = sphere(ctx)
    P, _ = sphere_camera(0.0)
    buf = check_depth(ctx, v, f, P, 96, 72, "sphere")
    ys, xs = np.mgrid[0:72, 0:96]
    rho = np.hypot(xs - 48.0, ys - 36.0)                     # the outline: radius 150 * 50 / sqrt(250^2 - 50^2) = 30.6 pixels
    assert (buf[rho < 29.0] != 0).all() and (buf[rho > 32.0] == 0).all()
    P2, _ = sphere_camera(130.0, -35.0, dist=120.0, fx=60.0)
    check_depth(ctx, v, f, P2, 96, 72, "sphere, near and oblique")


def test_depth_buffer_big_box_tier_equals_the_thread_tier(ctx):
    v, f = big_scene()
    img = np.zeros((72, 96, 3), np.uint8)
    cams = [cam_pair(EYE_P, img, None, EYE_P, img, None)]
    a = check_depth(ctx, v, f, EYE_P, 96, 72, "big triangle behind small ones")
    assert (a != 0).all() and (a > np.float32(0.1).view(np.uint32)).sum() > 50      # the small ones are nearer than depth 10
    st = ctx.mesh_color(v, f, cams, 1.0)[2]
    assert st["items_big_box"] == 2 and st["items_drawn"] > 2 and st == mr.color(v, f, mr.views_of(cams), 1, 0.2, 1.0)[2]
    ctx.set_option("meshcolor_big_box", 1 << 20)             # everything in the thread tier: the same bytes
    try:
        b = ctx.mesh_depth(v, f, EYE_P, 96, 72)
        st2 = ctx.mesh_color(v, f, cams, 1.0)[2]
    finally:
        ctx.set_option("meshcolor_big_box", 4096)
    assert b.tobytes() == a.tobytes() and st2["items_big_box"] == 0 and st2["items_drawn"] == st["items_drawn"]
    ctx.set_option("meshcolor_big_box", 1)                   # and everything of more than one pixel in the block tier
    try:
        c = ctx.mesh_depth(v, f, EYE_P, 96, 72)
    finally:
        ctx.set_option("meshcolor_big_box", 4096)
    assert c.tobytes() == a.tobytes()


def test_depth_buffer_of_triangles_outside_behind_and_without_area(ctx):
    rng = np.random.default_rng(22)
    v = [[-300, 100, 5], [200, 50, 5], [100, 300, 5],        # partly outside on the left and below
         [400, -50, 4], [600, 300, 4], [300, 100, 4],        # partly outside on the right and above
         [10, 10, 2], [60, 10, 2], [30, 40, -1],             # a vertex behind the camera: skipped
         [10, 10, 2], [60, 10, 2], [30, 40, 0],              # a vertex on the camera plane: skipped
         [20, 20, 1], [40, 40, 2], [90, 90, 3],              # collinear in the image: no area
         [50, 50, 1], [50, 50, 1], [70, 90, 1],              # two equal vertices
         [-500, -500, 1], [-400, -500, 1], [-500, -400, 1],  # entirely outside
         [1e30, 0, 1e-9], [0, 1e30, 1e-9], [5, 5, 1]]        # quotients that overflow float: skipped
    f = np.arange(len(v)).reshape(-1, 3)
    v, f = np.float32(v), np.int32(f)
    buf = check_depth(ctx, v, f, EYE_P, 96, 72, "edge cases")
    assert (buf != 0).any()
    assert mr.depth_buffer(v, f[2:], EYE_P, 96, 72).any() == False   # noqa: E712  (all but the first two draw nothing)
    # a soup of random triangles of every size, some crossing the borders
    n = 400
    c = rng.uniform(-20, 116, (n, 1, 2)) + rng.uniform(-1, 1, (n, 3, 2)) * rng.choice([0.4, 3.0, 30.0, 120.0], (n, 1, 1))
    z = rng.uniform(1.0, 9.0, (n, 3, 1))
    sv = np.concatenate([c * z, z], axis=2).reshape(-1, 3).astype(np.float32)
    check_depth(ctx, sv, np.arange(3 * n, dtype=np.int32).reshape(-1, 3), EYE_P, 96, 72, "soup")


def test_depth_buffer_of_a_tessellated_quad_has_no_gaps(ctx):
    v, f = mr.grid_plane(29, 21, 3.0, 4.0, 3.0, 1.0)        # integer projections 3 .. 87 by 4 .. 64, depth 1
    buf = check_depth(ctx, v, f, EYE_P, 96, 72, "quad")
    ys, xs = np.mgrid[0:72, 0:96]
    inside = (xs >= 3) & (xs <= 87) & (ys >= 4) & (ys <= 64)
    assert np.array_equal(buf != 0, inside) and set(buf[inside].tolist()) == {int(np.float32(1.0).view(np.uint32))}
    # the same quad slanted in depth (integer projections still: x = u z, y = v z): every pixel centre inside it is drawn
    uu, vv = v[:, 0].astype(np.float64), v[:, 1].astype(np.float64)
    z = 2.0 + uu / 64.0 + vv / 32.0                          # dyadic: x, y and the quotients are exact in float
    sl = np.stack([uu * z, vv * z, z], axis=1).astype(np.float32)
    buf = check_depth(ctx, sl, f, EYE_P, 96, 72, "slanted quad")
    assert np.array_equal(buf != 0, inside)


# ---- 3: occlusion, a known answer ---------------------------------------------------------------------------------------------------------
def two_squares():
    """a 16 x 16 square at depth 20 behind a 4 x 4 square at depth 10, both facing the camera at the origin"""
    vb, fb = mr.grid_plane(17, 17, -8.0, -8.0, 1.0, 20.0)
    vf, ff = mr.grid_plane(5, 5, -2.0, -2.0, 1.0, 10.0)
    return vb, vf, np.concatenate([vb, vf]), np.ascontiguousarray(np.concatenate([fb, ff + len(vb)])[:, ::-1])


def test_a_front_square_hides_the_back_vertices_behind_it(ctx):
    vb, vf, v, f = two_squares()
    P = K96 @ EYE_P
    img = random_image(31, 96, 72)
    cams = [cam_pair(P, img, None, P, img, np.zeros((72, 96), np.uint8))]           # the second view sees nothing: one camera
    # the front square projects onto 38 .. 58 by 26 .. 46; a back vertex (x, y) onto (48 + 2.5 x, 36 + 2.5 y), its pixel is that rounded
    # half up: hidden exactly when |x| <= 4 and |y| <= 4 (x = 4 -> pixel 58, the front's edge, drawn; x = 5 -> 60.5 -> pixel 61)
    hidden = np.concatenate([(np.abs(vb[:, 0]) <= 4) & (np.abs(vb[:, 1]) <= 4), np.zeros(len(vf), bool)])
    px = np.floor(48 + 50 * v[:, 0].astype(np.float64) / v[:, 2] + 0.5).astype(int)
    py = np.floor(36 + 50 * v[:, 1].astype(np.float64) / v[:, 2] + 0.5).astype(int)
    for mode in (0, 1):
        rgb, best, st = ctx.mesh_color(v, f, cams, 1.0, mode=mode)
        assert hidden.sum() == 81 and np.array_equal(best == -1, hidden) and (best[~hidden] == 0).all()
        assert (rgb[hidden] == 127).all() and np.array_equal(rgb[~hidden], img[py[~hidden], px[~hidden]][:, ::-1])
        assert st["coloured"] == len(v) - 81 and st["visible_views"] == len(v) - 81 and st["no_normal"] == 0
    # a slack as deep as the gap lets them through
    assert (ctx.mesh_color(v, f, cams, 10.01)[1] == 0).all()
    assert (ctx.mesh_color(v, f, cams, 9.99)[1] == -1).sum() == 81


# ---- 4: the sphere between two opposite cameras ---------------------------------------------------------------------------------------------
def test_sphere_between_a_red_and_a_blue_camera(ctx):
    v, f, h = sphere(ctx)
    D, fx, W, H = 250.0, 150.0, 96, 72
    Pa, eye_a = sphere_camera(0.0)
    Pb, eye_b = sphere_camera(180.0)
    red, blue = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
    red[..., 2], blue[..., 0] = 255, 255
    cams = [cam_pair(Pa, red, None, Pb, blue, None)]
    eps = 2.0 * h
    r = v.astype(np.float64) - pr.SPHERE_C
    axis = (eye_a - pr.SPHERE_C) / D                         # towards camera a; camera b is at -axis
    za = r @ axis
    rad = np.linalg.norm(r, axis=1)
    # min_cos = 0.5: only the cap that faces a camera within 60 degrees; the band between the caps is grey
    rgb, best, st = ctx.mesh_color(v, f, cams, eps, mode=0, min_cos=0.5)
    assert (za[best == 0] > 0).all() and (za[best == 1] < 0).all()
    assert (rgb[best == 0] == [255, 0, 0]).all() and (rgb[best == 1] == [0, 0, 255]).all() and (rgb[best == -1] == 127).all()
    band = np.abs(za) < 0.2 * rad                            # there cos < 0.2 + (the mesh normal's deviation from the radius): far below 0.5
    assert band.sum() > 100 and (best[band] == -1).all()
    assert (best == 0).sum() > 0.15 * len(v) and (best == 1).sum() > 0.15 * len(v)
    # min_cos = -0.99: the cos test lets nearly everything through, so the depth test alone keeps a camera's colour off the far side.
    # A far-side vertex j at camera depth q2 = D - za and image radius rho is tested at a pixel centre at most sqrt(1/2) pixel from its
    # projection; the mesh is closed and encloses the sphere of radius r_in (the least vertex radius less the sag of a face,
    # edge^2 / (6 r)), so the buffer there holds a depth of at most z_in(rho + sqrt(1/2)), the first hit of that sphere -- increasing in
    # the radius.  The vertex must therefore be hidden when q2 > z_in(rho + sqrt(1/2)) + depth_eps (+ 1e-3 D for the float projection).
    edge = max(np.linalg.norm(v[f[:, a]].astype(np.float64) - v[f[:, b]], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    r_in = rad.min() - edge * edge / (6.0 * rad.min())
    rgb, best, st = ctx.mesh_color(v, f, cams, eps, mode=0, min_cos=-0.99)
    phi_s = np.arccos(pr.SPHERE_R / D)                       # the silhouette's polar angle from the camera's axis
    for view, zc in ((0, za), (1, -za)):
        lat = np.sqrt(np.maximum(rad * rad - zc * zc, 0.0))
        q2 = D - zc
        s = (fx * lat / q2 + np.sqrt(0.5) + 1e-3) / fx
        disc = D * D - (1 + s * s) * (D * D - r_in * r_in)
        z_in = (D - np.sqrt(np.maximum(disc, 0.0))) / (1 + s * s)
        must_hide = (disc > 0) & (q2 > z_in + eps + 1e-3 * D)
        past = np.arctan2(lat, zc) - phi_s                   # how far past the silhouette the vertex lies
        margin = past[~must_hide].max()                      # beyond this angle every vertex is in must_hide
        print("view %d: %d of %d vertices must be hidden (everything more than %.1f degrees past the silhouette); %d took its colour"
              % (view, must_hide.sum(), len(v), np.degrees(margin), (best == view).sum()))
        # (an ideal vertex on the radius 51 against r_in = 48.8 gives 21 degrees here, one on 49 gives 14: the bound below only keeps
        # the test from passing on an empty set)
        assert must_hide.sum() > 0.25 * len(v) and margin < np.radians(30.0)
        assert (best[must_hide] != view).all()
        assert not (rgb[must_hide] == ([255, 0, 0] if view == 0 else [0, 0, 255])).all(axis=1).any()


# ---- 5: a frontal plane on exact pixels -----------------------------------------------------------------------------------------------------
def test_frontal_plane_takes_the_pixels_it_projects_to(ctx):
    v, f = mr.grid_plane(17, 13, -8.0, -6.0, 1.0, 10.0)     # projects to 48 + 5 x, 36 + 5 y: 8 .. 88 by 6 .. 66
    f = np.ascontiguousarray(f[:, ::-1])
    img = random_image(51, 96, 72)
    P = K96 @ EYE_P
    cams = [cam_pair(P, img, None, P, img, None)]
    want = img[(36 + 5 * v[:, 1]).astype(int), (48 + 5 * v[:, 0]).astype(int)][:, ::-1]
    for mode in (0, 1):
        rgb, best, st = ctx.mesh_color(v, f, cams, 0.5, mode=mode)
        assert np.array_equal(rgb, want) and (best == 0).all() and st["visible_views"] == 2 * len(v)
    assert len(np.unique(want, axis=0)) > 200 and (want[:, 0] != want[:, 2]).any()


# ---- 6: both modes against the restatement ------------------------------------------------------------------------------------------------
def four_views():
    W, H = 128, 96
    Ps = [sphere_camera(a, e, dist=d, fx=fx, W=W, H=H)[0] for a, e, d, fx in ((0, 10, 250, 200), (20, -15, 230, 190), (95, 5, 300, 260), (200, 40, 220, 150))]
    rng = np.random.default_rng(61)
    masks = []
    for k in range(4):
        m = np.full((H, W), 255, np.uint8)
        for _ in range(6):
            x, y = rng.integers(20, W - 30), rng.integers(15, H - 25)
            m[y:y + 12, x:x + 14] = rng.choice([0, 128])
        masks.append(m)
    masks[2] = None
    imgs = [random_image(62 + k, W, H) for k in range(4)]
    # views 0 .. 3 = pair 0 view 0, pair 1 view 0, pair 0 view 1, pair 1 view 1
    return [cam_pair(Ps[0], imgs[0], masks[0], Ps[2], imgs[2], masks[2]), cam_pair(Ps[1], imgs[1], masks[1], Ps[3], imgs[3], masks[3])]


def test_both_modes_on_the_sphere_with_four_views_equal_the_restatement(ctx):
    v, f, h = sphere(ctx)
    cams = four_views()
    views = mr.views_of(cams)
    assert views[1][0] is cams[1][0].P and views[2][2] is None
    e0, e1, ebest, est = mr.color(v, f, views, "both", 0.2, 2.0 * h)
    for mode, want in ((0, e0), (1, e1)):
        rgb, best, st = ctx.mesh_color(v, f, cams, 2.0 * h, mode=mode)
        print("mode %d: %s; colours that differ: %d, best views that differ: %d" % (mode, st, (rgb != want).any(axis=1).sum(), (best != ebest).sum()))
        assert rgb.tobytes() == want.tobytes() and best.tobytes() == ebest.tobytes() and st == est
    assert set(np.unique(ebest).tolist()) == {-1, 0, 1, 2, 3} and est["visible_views"] > est["coloured"] > 0.5 * len(v)
    assert (e0 != e1).any()
    # another threshold and slack, and a min_cos below zero
    for min_cos, eps in ((0.6, 0.0), (-0.5, 0.25 * h)):
        rgb, best, st = ctx.mesh_color(v, f, cams, eps, mode=1, min_cos=min_cos)
        w1, wb, ws = mr.color(v, f, views, 1, min_cos, eps)
        assert rgb.tobytes() == w1.tobytes() and best.tobytes() == wb.tobytes() and st == ws


def test_two_camera_plane_gives_the_closed_form_blend(ctx):
    v, f = mr.grid_plane(9, 7, -4.0, -3.0, 1.0, 0.0)        # the plane z = 0, normal +z
    W, H = 64, 48
    ea, eb = np.array([3.0, -2.0, 100.0]), np.array([70.0, 10.0, 60.0])
    Pa, Pb = mr.look_at(ea, (0, 0, 0), 400.0, 32.0, 24.0), mr.look_at(eb, (0, 0, 0), 400.0, 32.0, 24.0)
    ca, cb = np.array([200, 10, 60]), np.array([20, 250, 90])
    ia, ib = np.empty((H, W, 3), np.uint8), np.empty((H, W, 3), np.uint8)
    ia[:], ib[:] = ca[::-1], cb[::-1]
    rgb, best, st = ctx.mesh_color(v, f, [cam_pair(Pa, ia, None, Pb, ib, None)], 0.5, mode=1)
    p = v.astype(np.float64)
    cosa = (ea - p)[:, 2] / np.linalg.norm(ea - p, axis=1)
    cosb = (eb - p)[:, 2] / np.linalg.norm(eb - p, axis=1)
    real = (cosa[:, None] * ca + cosb[:, None] * cb) / (cosa + cosb)[:, None]
    assert (np.abs(rgb.astype(np.float64) - real) <= 0.5 + 1e-9).all() and (best == 0).all() and st["visible_views"] == 2 * len(v)
    assert len(np.unique(rgb, axis=0)) > 5                   # the weights vary over the plane


# ---- 7: entry points, reproducibility, refusals ---------------------------------------------------------------------------------------------
def test_host_device_and_last_entries_return_the_same_bytes(ctx):
    xyz, nrm = pr.sphere_samples(20000)
    v, f, pst = ctx.poisson_mesh(xyz, nrm, 5, trim_cells=0)  # the context's last mesh
    cams = four_views()
    eps = 2.0 * pst["h"]
    a = ctx.mesh_color(v, f, cams, eps)
    b = ctx.mesh_color(v, f, cams, eps)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[2]["coloured"] > 1000
    dv, df = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    drgb = torch.zeros((len(v), 3), dtype=torch.uint8, device="cuda")
    dbest = torch.zeros(len(v), dtype=torch.int32, device="cuda")
    st = ctx.mesh_color_device(dv.data_ptr(), len(v), df.data_ptr(), len(f), cams, drgb.data_ptr(), dbest.data_ptr(), eps)
    torch.cuda.synchronize()
    assert drgb.cpu().numpy().tobytes() == a[0].tobytes() and dbest.cpu().numpy().tobytes() == a[1].tobytes() and st == a[2]
    st = ctx.mesh_color_device(dv.data_ptr(), len(v), df.data_ptr(), len(f), cams, drgb.data_ptr(), 0, eps)       # best_view may be NULL
    assert st == a[2]
    c = ctx.mesh_color_last(cams, eps)
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes() and c[2] == a[2]
    lv, lf = ctx.poisson_last_mesh(len(v), len(f))           # the mesh itself is untouched
    assert lv.tobytes() == v.tobytes() and lf.tobytes() == f.tobytes()
    # a new mesh has no colours until it is coloured
    from reconstruction_amd import RsmError
    ctx.mesh_clean_last(smooth_steps=1)
    with pytest.raises(RsmError) as e:
        ctx._chk(ctx._lib.rsm_mesh_last_colors(ctx._h, None, None))
    assert e.value.code == -5 and "colours" in str(e.value)


def test_the_empty_mesh(ctx):
    cams = four_views()
    e = np.zeros((0, 3))
    rgb, best, st = ctx.mesh_color(e, e, cams, 1.0)
    assert rgb.shape == (0, 3) and best.shape == (0,) and st == mr.color(e, e, mr.views_of(cams), 1, 0.2, 1.0)[2] and st["n_vertices"] == 0
    assert ctx.mesh_color(e, e, [], 1.0)[2]["n_vertices"] == 0                     # no views are needed for no vertices
    assert not ctx.mesh_depth(e, e, EYE_P, 16, 8).any()
    v, f = mr.grid_plane(3, 3, 0.0, 0.0, 1.0, 5.0)
    rgb, best, st = ctx.mesh_color(v, e, cams, 1.0)          # vertices without faces: no normals, nothing coloured
    assert (rgb == 127).all() and (best == -1).all() and st["no_normal"] == 9 and st == mr.color(v, e, mr.views_of(cams), 1, 0.2, 1.0)[2]


def test_invalid_input_is_refused_and_named(ctx):
    from reconstruction_amd._lib import RSM_E_INVALID, MeshColorParams
    lib, h = ctx._lib, ctx._h
    v, f = mr.grid_plane(5, 5, -2.0, -2.0, 1.0, 10.0)
    img = np.zeros((72, 96, 3), np.uint8)
    P = K96 @ EYE_P
    good = [cam_pair(P, img, None, P, img, None)]
    rgb, best = np.zeros((len(v), 3), np.uint8), np.zeros(len(v), np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(V=v, F=f, cams=good, n_pairs=None, views="cams", params="p", out=rgb, n_v=None, n_f=None, edit=None, **kw):
        p = MeshColorParams(1, 0.2, 1.0)
        for k, val in kw.items():
            setattr(p, k, val)
        vw, keep = ctx.mesh_color_views(cams)
        if edit:
            edit(vw)
        st = lib.rsm_mesh_color(h, ptr(V), C.c_int64(len(V) if n_v is None else n_v), ptr(F), C.c_int64(len(F) if n_f is None else n_f),
                                vw if views == "cams" else None, C.c_int(len(cams) if n_pairs is None else n_pairs),
                                C.byref(p) if params == "p" else None, ptr(out), ptr(best), None)
        return st, (lib.rsm_last_error(h) or b"").decode()
    bad_i, neg_i, bad_c, inf_c = f.copy(), f.copy(), v.copy(), v.copy()
    bad_i[7, 1] = len(v)
    neg_i[0, 0] = -1
    bad_c[3, 2] = np.nan
    inf_c[24, 0] = np.inf
    sing = P.copy()
    sing[2, :3] = 2.0 * sing[0, :3]

    def set_field(name, val):
        return lambda vw: setattr(vw[0], name, val)

    def null_image(vw):
        vw[0].image[1] = None
    for kw, name in ((dict(F=bad_i), "index"), (dict(F=neg_i), "index"), (dict(V=bad_c), "finite"), (dict(V=inf_c), "finite"),
                     (dict(n_f=(2 ** 31 + 2) // 3), "nf"), (dict(n_f=-1), "nf"), (dict(n_v=-1), "nv"), (dict(n_v=2 ** 31), "nv"),
                     (dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(min_cos=1.0), "min_cos"), (dict(min_cos=-1.5), "min_cos"),
                     (dict(min_cos=float("nan")), "min_cos"), (dict(depth_eps=-0.1), "depth_eps"), (dict(depth_eps=float("inf")), "depth_eps"),
                     (dict(depth_eps=float("nan")), "depth_eps"), (dict(params=None), "params"), (dict(n_pairs=0), "n_pairs"),
                     (dict(views=None), "NULL"), (dict(V=None, n_v=len(v)), "NULL"), (dict(F=None, n_f=len(f)), "NULL"), (dict(out=None), "NULL"),
                     (dict(edit=null_image), "NULL"), (dict(edit=set_field("width", 0)), "width"), (dict(edit=set_field("height", -3)), "height"),
                     (dict(cams=[cam_pair(P, img, None, sing, img, None)]), "singular")):
        st, msg = call(**kw)
        assert st == RSM_E_INVALID and name in msg, (kw, st, msg)
    assert call()[0] == 0 and call(min_cos=-1.0, depth_eps=0.0, mode=0)[0] == 0
    # the other entries check the same inputs
    from reconstruction_amd import RsmError
    for fn in (lambda: ctx.mesh_depth(v, bad_i, P, 96, 72), lambda: ctx.mesh_depth(bad_c, f, P, 96, 72), lambda: ctx.mesh_depth(v, f, P, 0, 72),
               lambda: ctx.mesh_color(v, neg_i, good, 1.0), lambda: ctx.mesh_color_last(good, -1.0), lambda: ctx.mesh_color_last(good, 1.0, mode=3),
               lambda: ctx.mesh_color_device(0, len(v), 0, 0, good, 0, 0, 1.0),
               lambda: ctx._chk(lib.rsm_texture_color(h, ptr(v), C.c_int64(len(v)), ptr(np.ascontiguousarray(P)), ptr(img), 0, 72, ptr(rgb))),
               lambda: ctx._chk(lib.rsm_texture_color(h, ptr(v), C.c_int64(len(v)), ptr(np.ascontiguousarray(P)), None, 96, 72, ptr(rgb)))):
        with pytest.raises(RsmError) as e:
            fn()
        assert e.value.code == RSM_E_INVALID


# ---- 8: end to end ------------------------------------------------------------------------------------------------------------------------
def test_cloud_optimization_run_mesh_clean_mesh_then_color_mesh(ctx):
    from reconstruction_amd import CloudOptimization, ManageData, StereoMatching
    # The rig: test_cloud_optimization_run_mesh_then_clean_mesh's two small pairs (4 and 5, disparity 12 +- 8 pixels) do not serve here.
    # synth alternates the disparity's sign with the pair, and with Q's sign (Z = -f B / d) an even pair's cloud lies at negative depth,
    # behind its own cameras, where nothing is visible; and a disparity of 12 +- 8 pixels is a depth of 1 920 .. 9 600, a surface that
    # is seen at a grazing angle nearly everywhere (the restatement colours 659 of that mesh's 6 448 vertices).  So: two odd pairs
    # (d < 0, in front of their cameras), disparity 12 +- 1 pixels (depth 2 950 .. 3 490, seen almost frontally), wider masks, and a trim
    # of 2 cells, so that the rim of the surface beyond the masks (never coloured) stays narrow.
    cfgs = [synth.config_small(320, 192, 3, radius=2, pair=5, mask_l0_width=70, border_l0=2, amp_l0=0.25),
            synth.config_small(320, 192, 3, radius=2, pair=7, mask_l0_width=70, border_l0=2, amp_l0=0.25, holes=True)]
    top = 1 << (cfgs[0].pyr_levels - 1)
    cams = []
    for c in cfgs:                                           # the cameras given P, so that colouring is possible
        P0, P1, centre = synth.rectified_views(c.Q, c.R_final, c.T_final)
        cams.append([Camera(camID=0, image=c.image[0], mask=c.mask[0], CamCenter=centre, P=P0),
                     Camera(camID=1, image=c.image[1], mask=c.mask[1], CamCenter=centre, P=P1)])
    data = ManageData(cam=cams, m_PyrmNum=cfgs[0].pyr_levels, m_LowestLevelSize=(cfgs[0].width // top, cfgs[0].height // top),
                      m_OriginSize=(cfgs[0].width, cfgs[0].height), rectified=[dict(Q=c.Q, R_final=c.R_final, T_final=c.T_final) for c in cfgs])
    opt = CloudOptimization(ctx)
    opt.Init(100, 1, 50, 2, 40.0, data, False)
    sm = StereoMatching(0)
    sm.Init(data, opt, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    opt.run()
    with pytest.raises(ValueError, match="mesh"):
        opt.color_mesh()
    _, _, mst = opt.mesh(depth=7, trim_cells=2)
    v, f, _ = opt.clean_mesh()
    rgb, best, st = opt.color_mesh()
    assert opt.mesh_colors[0] is rgb and opt.mesh_result[0] is v
    views = mr.views_of(cams)
    e0, e1, ebest, est = mr.color(v, f, views, "both", 0.2, 2.0 * mst["h"])
    print("run() -> mesh() -> clean_mesh() -> color_mesh(): %s" % st)
    assert rgb.tobytes() == e1.tobytes() and best.tobytes() == ebest.tobytes() and st == est
    assert est["coloured"] > 0.5 * len(v)
    rgb0, best0, st0 = opt.color_mesh(mode=0, min_cos=0.3, depth_eps=1.5)
    w0, wb, ws = mr.color(v, f, views, 0, 0.3, 1.5)
    assert rgb0.tobytes() == w0.tobytes() and best0.tobytes() == wb.tobytes() and st0 == ws
    hv, hf = ctx.poisson_last_mesh(len(v), len(f))           # the mesh is untouched
    assert hv.tobytes() == v.tobytes() and hf.tobytes() == f.tobytes()
    cams[1][1].P = None                                      # pre-rectified input carries no P
    with pytest.raises(ValueError, match="pre-rectified input carries no P"):
        opt.color_mesh()


# ---- 9: the command line --------------------------------------------------------------------------------------------------------------------
def read_ply_mesh_color(path):
    with open(path, "rb") as fp:
        head = b""
        while not head.endswith(b"end_header\n"):
            head += fp.readline()
        lines = head.decode().splitlines()
        nv, nf = int(lines[2].split()[2]), int([l for l in lines if l.startswith("element face")][0].split()[2])
        assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
        assert [l for l in lines if l.startswith("property")] == ["property float x", "property float y", "property float z", "property uchar red",
                                                                  "property uchar green", "property uchar blue",
                                                                  "property list uchar int vertex_indices"]
        rec = np.frombuffer(fp.read(15 * nv), np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
        fr = np.frombuffer(fp.read(13 * nf), np.dtype([("n", "u1"), ("i", "<i4", 3)]))
        assert fp.read() == b"" and (fr["n"] == 3).all()
        return rec["p"].copy(), fr["i"].astype(np.int32).reshape(nf, 3), rec["c"].copy()


def test_cli_mesh_color_writes_the_coloured_mesh_to_outfilename(ctx, tmp_path, capsys):
    from PIL import Image
    from reconstruction_amd import StereoMatching
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
    base = [root + "config.yml", "--mls-radius", "10", "--mesh-depth", "7", "--mesh-clean"]
    capsys.readouterr()
    assert main(base) == 0                                   # without the flag: out.ply is the cloud
    plain = norm(capsys.readouterr().out).splitlines()
    cloud, mesh = open(root + "out.ply", "rb").read(), open(root + "bigmesh.ply", "rb").read()
    assert not any("colour" in l for l in plain) and cloud.startswith(b"ply") and b"property uchar blue\nproperty uchar green" in cloud[:400]
    assert main(base + ["--mesh-color"]) == 0
    out = norm(capsys.readouterr().out).splitlines()
    assert open(root + "bigmesh.ply", "rb").read() == mesh and open(root + "out_cloud.ply", "rb").read() == cloud
    # every line but the cloud's path and the one added line is what it was
    assert out[:-1] == [l.replace(root + "out.ply", root + "out_cloud.ply") for l in plain]
    v, f, rgb = read_ply_mesh_color(root + "out.ply")
    mv, mf = pr.read_ply_mesh(root + "bigmesh.ply")
    assert v.tobytes() == mv.tobytes() and np.array_equal(f, mf)
    # the views as the command rectified them, and the grid step from the mesh's own statistics
    data, _ = cfgmod.load_config(root + "config.yml")
    sm = StereoMatching(0)
    sm.Init(data, None, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    h = _grid_step(ctx, root)
    want, wbest, wst = mr.color(mv, mf, mr.views_of(data.cam), 1, 0.2, 2.0 * h)
    assert rgb.tobytes() == want.tobytes()
    assert out[-1] == "Mesh colour: %d of %d vertices coloured from 2 views (%d without a normal) -> %sout.ply" % (wst["coloured"], len(mv), wst["no_normal"], root)
    assert wst["coloured"] > 0
    # the options
    assert main(base + ["--mesh-color", "--mesh-color-mode", "best", "--mesh-color-min-cos", "0.4", "--mesh-color-eps", "3.5", "--out", root + "c.ply"]) == 0
    capsys.readouterr()
    assert open(root + "c.ply", "rb").read() == cloud
    assert read_ply_mesh_color(root + "out.ply")[2].tobytes() == mr.color(mv, mf, mr.views_of(data.cam), 0, 0.4, 3.5)[0].tobytes()
    assert main(base + ["--mesh-color", "--mesh-color-min-cos", "1.5"]) == 1
    assert "min_cos" in capsys.readouterr().out


def _grid_step(ctx, root):
    """the Poisson grid step of the command's mesh: the surface of bigcloud.ply (what --mesh reads) at the command's depth"""
    rec = np.frombuffer(open(root + "bigcloud.ply", "rb").read().split(b"end_header\n", 1)[1], "<f4").reshape(-1, 7)
    return ctx.poisson_mesh(rec[:, :3], rec[:, 3:], 7, trim_cells=4)[2]["h"]
