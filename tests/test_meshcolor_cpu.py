"""The numpy restatement of the mesh colouring (tests/meshcolor_restatement.py) against answers worked out by hand: it
is the judge of csrc/k_meshcolor.hip (tests/test_gpu_meshcolor.py), so it is itself tested here, without a GPU."""
import numpy as np

import meshcolor_restatement as mr

EYE_P = np.hstack([np.eye(3), np.zeros((3, 1))])            # pixel = (x / z, y / z), centre at the origin


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_texture_color_pixels_by_hand():
    W, H = 8, 6
    img = np.zeros((H, W, 3), np.uint8)
    img[..., 0] = 10 + np.arange(W)[None, :]                 # blue  = 10 + x
    img[..., 1] = 100 + np.arange(H)[:, None]                # green = 100 + y
    img[..., 2] = 200                                        # red
    grey = [127, 127, 127]
    cases = [((3.2, 1.6, 1.0), [200, 102, 13]),              # ROUND(3.2) = 3, ROUND(1.6) = 2; BGR -> RGB
             ((6.4, 3.2, 2.0), [200, 102, 13]),              # the same pixel from twice the depth
             ((-0.7, 0.0, 1.0), [200, 100, 10]),             # (int)(-0.7 + 0.5) = (int)(-0.2) = 0: pixel 0
             ((0.0, -1.4, 1.0), [200, 100, 10]),             # (int)(-0.9) = 0
             ((-1.5, 0.0, 1.0), grey),                       # (int)(-1.0) = -1: outside
             ((7.4, 5.4, 1.0), [200, 105, 17]),              # the last pixel
             ((7.5, 0.0, 1.0), grey),                        # ROUND = 8 = W
             ((0.0, 5.5, 1.0), grey),                        # ROUND = 6 = H
             ((-3.0, -2.0, -1.0), [200, 102, 13]),           # behind the camera: no test of the depth's sign
             ((1.0, 1.0, 0.0), grey),                        # q2 = 0: the quotient is not finite
             ((0.0, 0.0, 0.0), grey),                        # 0 / 0
             ((np.nan, 0.0, 1.0), grey),
             ((1e30, 0.0, 1e-9), grey)]                      # the quotient overflows float / int
    got = mr.texture_color(np.float32([c[0] for c in cases]), EYE_P, img)
    assert got.tolist() == [c[1] for c in cases]


def test_one_triangle_coverage_and_inverse_depth_by_hand():
    # (u, v) = (0, 0), (4, 0), (0, 4) at depth 2: the 15 pixel centres with x + y <= 4, edges included, w = 1 / 2
    v = np.float32([[0, 0, 2], [8, 0, 2], [0, 8, 2]])
    for f in ([[0, 1, 2]], [[0, 2, 1]]):                     # both orientations are drawn
        buf, drawn, big = mr.depth_buffer(v, f, EYE_P, 8, 6, True)
        ys, xs = np.mgrid[0:6, 0:8]
        assert np.array_equal(buf != 0, xs + ys <= 4) and (buf != 0).sum() == 15 and (drawn, big) == (1, 0)
        assert set(buf[buf != 0].tolist()) == {bits(0.5)}
    # depths 1, 2, 2: w = (1, 1/2, 1/2) at the corners; at (1, 1) lambda = (1/2, 1/4, 1/4): w = 3/4
    v = np.float32([[0, 0, 1], [8, 0, 2], [0, 8, 2]])
    buf = mr.depth_buffer(v, [[0, 1, 2]], EYE_P, 8, 6)
    assert buf[0, 0] == bits(1.0) and buf[0, 4] == bits(0.5) and buf[4, 0] == bits(0.5) and buf[1, 1] == bits(0.75) and buf[2, 2] == bits(0.5)
    assert buf[3, 2] == 0
    # nearer wins whatever the order; a vertex behind the camera, no area, a box outside the image: nothing
    two = np.float32([[0, 0, 2], [8, 0, 2], [0, 8, 2], [0, 0, 4], [32, 0, 4], [0, 32, 4]])
    a = mr.depth_buffer(two, [[0, 1, 2], [3, 4, 5]], EYE_P, 8, 6)
    b = mr.depth_buffer(two, [[3, 4, 5], [0, 1, 2]], EYE_P, 8, 6)
    assert np.array_equal(a, b) and a[0, 0] == bits(0.5) and a[3, 3] == bits(0.25)
    none = np.float32([[0, 0, 2], [8, 0, 2], [0, 8, -2], [1, 1, 1], [2, 2, 1], [3, 3, 1], [-9, -9, 1], [-5, -9, 1], [-9, -5, 1]])
    buf, drawn, big = mr.depth_buffer(none, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], EYE_P, 8, 6, True)
    assert not buf.any() and drawn == 0
    # the big-box count: a box of more pixels than big_box
    assert mr.depth_buffer(v, [[0, 1, 2]], EYE_P, 8, 6, True, big_box=24)[2] == 1
    assert mr.depth_buffer(v, [[0, 1, 2]], EYE_P, 8, 6, True, big_box=25)[2] == 0


def test_a_tessellated_quad_with_integer_projections_is_watertight():
    v, f = mr.grid_plane(7, 5, 2.0, 3.0, 3.0, 1.0)          # projections 2, 5, ..., 20 by 3, 6, ..., 15
    buf = mr.depth_buffer(v, f, EYE_P, 32, 24)
    ys, xs = np.mgrid[0:24, 0:32]
    inside = (xs >= 2) & (xs <= 20) & (ys >= 3) & (ys <= 15)
    assert np.array_equal(buf != 0, inside)
    assert set(buf[inside].tolist()) == {bits(1.0)}          # every pixel, shared edges and corners included, holds 1 / z exactly
    rng = np.random.default_rng(5)
    assert np.array_equal(mr.depth_buffer(v, f[rng.permutation(len(f))], EYE_P, 32, 24), buf)


def test_camera_centre_of_a_look_at_camera():
    for eye, target in (((250.0, -30.0, 40.0), (10.0, -20.0, 600.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0)), ((-7.5, 3.25, 1000.0), (1.0, 2.0, 3.0))):
        P = mr.look_at(eye, target, 150.0, 48.0, 36.0)
        C = mr.cam_center(P)
        assert np.allclose(C, eye, rtol=0, atol=1e-9 * (1.0 + np.abs(eye).max()))
        assert np.allclose(P @ np.append(C, 1.0), 0.0, atol=1e-7)      # the centre is P's null vector
    assert np.array_equal(mr.cam_center(EYE_P), np.zeros(3))
    sing = EYE_P.copy()
    sing[2, :3] = sing[0, :3]
    assert mr.cam_center(sing) is None


def test_vertex_normals_and_their_order():
    v, f = mr.grid_plane(3, 3, 0.0, 0.0, 2.0, 5.0)
    f = np.concatenate([f, [[4, 4, 0]]]).astype(np.int32)    # a repeated index takes no part
    N = mr.vertex_normals(v, f)
    assert np.array_equal(N[:, :2], np.zeros((9, 2))) and (N[:, 2] > 0).all()
    assert N[4, 2] == 6 * 4.0 and N[0, 2] == 2 * 4.0 and N[2, 2] == 4.0   # the centre meets six faces, corner 0 two, corner 2 one
    assert not mr.vertex_normals(v, np.zeros((0, 3), np.int32)).any()


def test_the_blends_weights_and_rounding():
    # a plane seen from straight above (cos = 1) and from 60 degrees (cos = 1/2), constant colours 100 and 201:
    # (1 * 100 + 0.5 * 201) / 1.5 = 133.67 -> 134; best view: the frontal one
    v, f = mr.grid_plane(3, 3, -1.0, -1.0, 1.0, 0.0)
    up, W, H = (0.0, 1.0, 0.0), 64, 48
    Pa = mr.look_at((0.0, 0.0, 100.0), (0.0, 0.0, 0.0), 400.0, 32.0, 24.0, up)
    Pb = mr.look_at((100.0 * np.sin(np.pi / 3), 0.0, 100.0 * np.cos(np.pi / 3)), (0.0, 0.0, 0.0), 400.0, 32.0, 24.0, up)
    ia, ib = np.full((H, W, 3), 100, np.uint8), np.full((H, W, 3), 201, np.uint8)
    ib[..., 0] = 1                                            # blue 1, green / red 201
    views = [(Pa, ia, None), (Pb, ib, None)]
    rgb0, rgb1, best, st = mr.color(v, f, views, "both", 0.2, 0.5)
    assert (best[4], rgb0[4].tolist(), rgb1[4].tolist()) == (0, [100, 100, 100], [134, 134, 67])   # (100 + 0.5) / 1.5 = 67
    assert (best == 0).all() and st["coloured"] == 9 and st["visible_views"] == 18 and st["no_normal"] == 0 and st["items_drawn"] == 16
    # min_cos above 1/2 shuts the oblique view out: the blend is the frontal colour
    rgb, best, st = mr.color(v, f, views, 1, 0.6, 0.5)
    assert (rgb == 100).all() and st["visible_views"] == 9
    # a view that faces the plane's back is let in by min_cos < 0 but carries no weight; alone, it gives its own colour
    Pc = mr.look_at((0.0, 60.0, -80.0), (0.0, 0.0, 0.0), 400.0, 32.0, 24.0, (1.0, 0.0, 0.0))   # cos = -0.8
    ic = np.full((H, W, 3), 7, np.uint8)
    rgb, best, st = mr.color(v, f, [(Pa, ia, None), (Pc, ic, None)], 1, -0.99, 0.5)
    assert (rgb == 100).all() and (best == 0).all() and st["visible_views"] == 18
    rgb, best, st = mr.color(v, f, [(Pc, ic, None), (Pc, ic, None)], 1, -0.99, 0.5)
    assert (rgb == 7).all() and (best == 0).all()
    # nothing visible: grey, -1
    rgb, best, st = mr.color(v, f, [(Pc, ic, None), (Pc, ic, None)], 1, 0.2, 0.5)
    assert (rgb == 127).all() and (best == -1).all() and st["coloured"] == 0


def test_a_front_square_hides_what_lies_behind_it():
    K = np.array([[50.0, 0, 48.0], [0, 50.0, 36.0], [0, 0, 1.0]])
    P = K @ EYE_P
    vb, fb = mr.grid_plane(17, 17, -8.0, -8.0, 1.0, 20.0)
    vf, ff = mr.grid_plane(5, 5, -2.0, -2.0, 1.0, 10.0)
    v, f = np.concatenate([vb, vf]), np.concatenate([fb, ff + len(vb)])[:, ::-1]          # normals towards the camera at the origin
    img = np.random.default_rng(1).integers(0, 256, (72, 96, 3)).astype(np.uint8)
    rgb, best, st = mr.color(v, f, [(P, img, None), (P, img, np.zeros((72, 96), np.uint8))], 0, 0.2, 1.0)
    hidden = np.concatenate([(np.abs(vb[:, 0]) <= 4) & (np.abs(vb[:, 1]) <= 4), np.zeros(len(vf), bool)])
    assert hidden.sum() == 81 and np.array_equal(best == -1, hidden) and (best[~hidden] == 0).all() and (rgb[hidden] == 127).all()
