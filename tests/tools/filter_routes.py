"""Which route the pair filter takes on a few synthetic pairs at k = 3 .. 128, and a digest of what it returns (records, normals,
statistics): `python tests/tools/filter_routes.py` from the root of a built tree, on the GPU.  Run from two built trees, the two outputs
compare the libraries route by route (profiles/f19_backend_refactor_routes.log)."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from reconstruction_amd import Context, synth

PAIRS = [dict(width=512, height=384, levels=5, radius=3, offset=2, pair=21, mask_l0_width=16, holes=True, occlude=True),
         dict(width=320, height=160, levels=2, radius=4, pair=7, mask_l0_width=100, border_l0=6, occlude=True),
         dict(width=256, height=192, levels=3, radius=2, pair=5, mask_l0_width=40, border_l0=4, holes=True),
         dict(width=320, height=192, levels=3, radius=2, pair=4, mask_l0_width=60, border_l0=4)]
with Context(0) as ctx:
    for ci, p in enumerate(PAIRS):
        res = ctx.match_pair(synth.config_small(**p))
        for k in (3, 8, 15, 30, 60, 100, 128):
            for fl in (23, 7):
                ctx.set_option("filter_list", fl)
                rec, nrm, st = ctx.filter_last_cloud_host(k, 1.0, 2.5, (1.0, -2.0, 1.0))
                info = ctx.filter_last_info()
                h = hashlib.sha1(rec.tobytes() + nrm.tobytes() + repr((st["mean"], st["stddev"], st["threshold"])).encode()).hexdigest()[:16]
                print("case %d k %3d filter_list %2d: radius %2d undecided %5d exhaustive %5s kept %6d %s" % (
                    ci, k, fl, info["radius"], info["undecided"], st.get("exhaustive"), len(rec), h), flush=True)
        ctx.set_option("filter_list", 23)
