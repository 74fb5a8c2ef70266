"""The fixtures of tests/test_gpu_cloud_filter_range.py held to what they are for, on the CPU: the tie cloud's first mean distance
depends on the order of its sum and the oracle's is the ascending one; the wide clouds leave (or, the control, stay inside) the
range in which the library's parallel sums over the cloud are accepted -- the witness that the GPU test runs the host's
sequential branch, its `bad` flag included."""
import numpy as np
import pytest

import cloud_range_fixtures as crf
from oracle import oracle as orc

# why the library's host has to refuse the parallel sums over each variant's distances (measured on the oracle's distances).  The
# far points and the cluster larger than k stretch the per-point means themselves; the cluster smaller than k and the
# underflowing points do not -- a member's k nearest reach the sheet, so its mean is an ordinary value: what those two stretch is the
# k-nearest sum of each member, the rule the kernels test per query.
STATS_WHY = {"far1e6": {"sq_sum"}, "far1e9": {"sq_sum"}, "far1e20": {"bad"}, "tight": {"sum", "sq_sum"}}     # (at least these)
PER_QUERY = ("tight_small", "underflow")


def test_tie_cloud_is_order_dependent_and_the_oracle_adds_ascending():
    xyz = crf.tie_cloud()
    keep, dist, stats = orc.sor_filter(xyz, crf.TIE_K, 1.0)
    assert float(dist[0]) == crf.TIE_DIST0 == float.fromhex("0x1.a00002p-1")
    orders = crf.tie_orders()
    assert len(orders) == 21                                   # 7! / (2! 5!) distinct orders of the seven values below the largest
    results = sorted(set(orders.values()))
    print("tie cloud: %d orders, results %s (%d / %d of them)" % (len(orders), [r.hex() for r in results],
                                                                  *(sum(v == r for v in orders.values()) for r in results)))
    assert len(results) == 2
    vals, last = crf.tie_values()
    assert vals == sorted(vals) and crf.sequential_mean(vals, last, crf.TIE_K) == float(dist[0])
    # the fixture's values are the cloud's, and the rule says this sum's order matters
    roots = crf.knn_roots(xyz, 0, crf.TIE_K)
    assert roots.tolist() == [float(v) for v in vals] + [float(last)]
    assert not crf.sum_is_order_free(roots)
    assert float(crf.dist2_f32(xyz[0], xyz[1:2])[0]) < 2.0 ** -96      # outside the trimmed square root's domain


@pytest.mark.parametrize("name", [name for name, _, _ in crf.wide_clouds()])
def test_wide_clouds_leave_the_parallel_sums_range(name):
    variant = name.split("-")[0]
    xyz, k = next((x, k) for nm, x, k in crf.wide_clouds() if nm == name)
    keep, dist, (mean, stddev, thr) = crf.wide_oracle(name)
    ok, why = crf.stats_fast_path(dist)
    print("%s: parallel sums %s%s; mean %r stddev %r threshold %r, %d kept" % (name, "accepted" if ok else "refused: ", why, mean, stddev, thr, int(keep.sum())))
    if variant in ("control",) + PER_QUERY:
        assert ok, why
    else:
        assert not ok and set(why.split("+")) >= STATS_WHY[variant], (why, STATS_WHY[variant])
    if variant == "far1e20":
        assert why == "bad" and np.isinf(mean) and np.isnan(thr) and keep.all()
    members = range(crf.WIDE_AT, crf.WIDE_AT + {"tight": k + 5, "tight_small": k - 3, "underflow": 12}.get(variant, 1))
    free = [crf.sum_is_order_free(crf.knn_roots(xyz, i, k)) for i in members]
    if variant in PER_QUERY:       # every member's own sum reaches from the cluster to the sheet: its order matters
        assert not any(free)
        for i in members:
            assert crf.sequential_mean(crf.knn_roots(xyz, i, k)[:-1], crf.knn_roots(xyz, i, k)[-1], k) == float(dist[i])
    elif variant in ("control", "tight"):
        assert all(free)           # (a cluster larger than k keeps each member's k nearest inside it: a narrow range)
    if variant == "underflow":
        d2 = np.concatenate([crf.dist2_f32(xyz[i], xyz[members.start:members.stop]) for i in members])
        assert ((d2 > 0) & (d2 < 2.0 ** -126)).any() and (d2 == 0).sum() > 12      # subnormal squares, and zeros between distinct points
        assert len(np.unique(xyz[members.start:members.stop], axis=0)) == 12
