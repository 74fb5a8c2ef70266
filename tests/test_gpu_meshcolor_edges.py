"""GPU mesh colouring (csrc/k_meshcolor.hip) at the edges of its rules, against references that do not restate its
expressions (tests/meshcolor_exact.py, itself tested in tests/test_meshcolor_exact_cpu.py):
  (a) the depth raster (rsm_stage_mesh_depth) on every case there against the exact integer reference, under its two derived tie rules
      and caps -- 0 excused decisions on the dyadic and integer cases --, the two tiers at meshcolor_big_box = 12 on boxes of 12 and 13
      pixels with the counters held to the exact boxes;
  (b) visibility, best view and colour (rsm_mesh_color, both modes) on planar scenes whose answers are known beforehand: the depth test
      at equality and one float32 beyond, an undrawn pixel, the strict cos test at the double 0.8, mask 255 / 254 / 0, the view numbering
      v = k n_pairs + i with three pairs, and 80 views.
If a case fails, the kernel or DESIGN's wording is wrong; the references and the caps are not to be loosened."""
import numpy as np
import pytest

import meshcolor_exact as mx
from reconstruction_amd import Camera

pytestmark = pytest.mark.gpu

DEFAULT_BIG_BOX = 4096


# ---- (a) the raster -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mx.CASES)
def test_depth_raster_is_the_exact_raster(ctx, name):
    c = mx.case(name)
    mx.hold(name, ctx.mesh_depth(c.v, c.f, c.P, c.W, c.H), "mesh_depth")


def test_excused_share_over_all_cases():
    dec = sum(mx.case_reference(n).decisions for n in mx.CASES)
    exc = sum(mx.case_reference(n).excused for n in mx.CASES)
    print("all %d cases: %d decisions, %d excused" % (len(mx.CASES), dec, exc))
    assert dec > 200000 and exc <= mx.CAP_ALL * dec


def test_denormal_inverse_depth_is_kept(ctx):
    c = mx.case("denormal")
    got = ctx.mesh_depth(c.v, c.f, c.P, 2, 2)
    assert got.tolist() == [[0x00400000, 0x00400000], [0x00400000, 0]]      # 2^-127; a flushed conversion would read "nothing drawn"


@pytest.mark.parametrize("name", ["tier_switch", "image_257x3", "box"])
def test_tier_switch_same_bits_and_exact_counts(ctx, name):
    c, R = mx.case(name), mx.case_reference(name)
    img = np.zeros((c.H, c.W, 3), np.uint8)
    cams = [[Camera(camID=0, P=c.P, image=img, mask=None), Camera(camID=1, P=c.P, image=img, mask=None)]]    # two views of the same raster
    bufs, counts = {}, {}
    for big_box in (mx.TIER_BIG_BOX, 1, 1 << 20):
        ctx.set_option("meshcolor_big_box", big_box)
        try:
            bufs[big_box] = ctx.mesh_depth(c.v, c.f, c.P, c.W, c.H)
            st = ctx.mesh_color(c.v, c.f, cams, 1.0)[2]
        finally:
            ctx.set_option("meshcolor_big_box", DEFAULT_BIG_BOX)
        counts[big_box] = (st["items_drawn"], st["items_big_box"])
        want = R.items(big_box)
        print("%s, meshcolor_big_box %d: items drawn / in the block tier %s, from the exact boxes 2 x %s" % (name, big_box, counts[big_box], want))
        assert counts[big_box] == (2 * want[0], 2 * want[1])
        assert R.mismatches(bufs[big_box]) == 0
    assert bufs[1].tobytes() == bufs[mx.TIER_BIG_BOX].tobytes() == bufs[1 << 20].tobytes()
    assert ctx.mesh_depth(c.v, c.f, c.P, c.W, c.H).tobytes() == bufs[1].tobytes()          # and with the default restored
    if name == "tier_switch":
        assert counts[mx.TIER_BIG_BOX] == (26, 10) and counts[1] == (26, 24) and counts[1 << 20] == (26, 0)


# ---- (b) visibility and colour, known answers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mx.SCENES)
def test_visibility_scene_has_its_known_answer(ctx, name):
    s = mx.scenes()[name]
    cams = [[Camera(camID=k, P=P, image=img, mask=m) for k, (P, img, m) in enumerate(pair)] for pair in s.pairs]
    for mode in (0, 1):
        rgb, best, st = ctx.mesh_color(s.v, s.f, cams, s.depth_eps, mode=mode, min_cos=s.min_cos)
        mx.hold_scene(s, mode, rgb, best)
        assert st["no_normal"] == 0 and st["n_vertices"] == len(s.v)
    if name.startswith("undrawn"):
        assert st["items_drawn"] == 0                        # the edge-on face has no area in either image
        assert not ctx.mesh_depth(s.v, s.f, s.pairs[0][0][0], 16, 12).any()
    if name.startswith("many_views"):
        assert st["visible_views"] == 3 * 80                 # every view sees all three vertices
