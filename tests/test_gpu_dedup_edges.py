"""csrc/k_dedup.hip on the edge fixtures of tests/dedup_edge_fixtures.py, against the numpy restatement (tests/dedup_restatement.py):
indices array_equal and counters ==, as tests/test_gpu_dedup.py does -- nothing here is approximate.  The fixtures sit on
CurrentValue within an ulp of -1, best-pair ties, every small bucket pattern, buckets across the selection grid's wave and block
boundaries, 2^k key totals, pairs of unequal size with empty ones, and ROUND at the halves; tests/test_dedup_edges_cpu.py holds the
restatement to an independent bucket-list statement on the same fixtures and shows what each one reaches.

Out of scope (see dedup_edge_fixtures.py): the 64-bit key instantiation, the open Eigen reduction-order question, and the bounds the
entry refuses (test_gpu_dedup.py::test_invalid_arguments)."""
import functools

import numpy as np
import pytest
import torch

import dedup_bucket_lists as bl
import dedup_edge_fixtures as fx
import dedup_restatement as dr
from reconstruction_amd import Camera

pytestmark = pytest.mark.gpu


def cams_of(views):
    out = []
    for v in views:
        out.append([Camera(camID=0, P=v["P"][0], image=v["image"][0], mask=v["mask"][0], bound=tuple(v["bound"]),
                           CamCenter=np.asarray(v["C"], np.float32)),
                    Camera(camID=1, P=v["P"][1], image=v["image"][1], mask=v["mask"][1])])
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    xyz, nrm, views = fx.get(name)
    with np.errstate(all="ignore"):
        return dr.dedup(xyz, nrm, views)


def first_difference(name, got, want):
    """Where the outputs part: the position, and the bucket (pair, pixel, size, CurrentValue) of the point the restatement has there."""
    xyz, nrm, views = fx.get(name)
    k = next((t for t in range(min(len(got), len(want))) if got[t] != want[t]), min(len(got), len(want)))
    tr = {}
    with np.errstate(all="ignore"):
        bl.dedup(xyz, nrm, views, tr)
    where = {j: (i, X, Y, len(m)) for i, X, Y, m in tr["buckets"] for j in m}
    lines = ["%s: %d indices, the restatement has %d; first difference at output position %d" % (name, len(got), len(want), k)]
    for who, arr in (("kernel", got), ("restatement", want)):
        if k < len(arr) and int(arr[k]) in where:
            i, X, Y, size = where[int(arr[k])]
            lines.append("  %s: point %d, pair %d pixel (%d, %d), bucket of %d, CurrentValue %r, values per pair %s"
                         % (who, arr[k], i, X, Y, size, dr.current_value(views[i], X, Y), [float(t) for t in tr["values"][int(arr[k])]]))
    return "\n".join(lines)


def check(name, idx, st):
    ridx, rst = restated(name)
    if not np.array_equal(idx, ridx):
        msg = first_difference(name, idx, ridx)
        print(msg)
        pytest.fail(msg)
    assert st == rst, name


@pytest.mark.parametrize("name", list(fx.FIXTURES))
def test_fixture_matches_the_restatement_twice(ctx, name):
    xyz, nrm, views = fx.get(name)
    cams = cams_of(views)
    idx, st = ctx.dedup_cloud(xyz, nrm, cams)
    check(name, idx, st)
    idx2, st2 = ctx.dedup_cloud(xyz, nrm, cams)
    assert idx2.tobytes() == idx.tobytes() and st2 == st


@pytest.mark.parametrize("name", ["unequal_full", "unequal_empty_first", "unequal_empty_middle", "unequal_all_empty",
                                  "exhaustive_patterns", "exhaustive_extremes"])
def test_device_entry_on_records_with_the_gather(ctx, name):
    xyz, nrm, views = fx.get(name)
    cams = cams_of(views)
    n = len(xyz)
    rec = np.zeros((n, 4), np.float32)                    # rsm_point16 records: stride 4
    rec[:, :3] = xyz
    rec[:, 3] = np.arange(n).astype(np.uint32).view(np.float32)
    d_rec = torch.from_numpy(rec).cuda()
    d_nrm = torch.from_numpy(np.ascontiguousarray(nrm)).cuda()
    d_idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    o_rec = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    o_nrm = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    m, st = ctx.dedup_cloud_device(d_rec.data_ptr(), d_nrm.data_ptr(), n, cams, d_idx.data_ptr(), o_rec.data_ptr(), o_nrm.data_ptr())
    torch.cuda.synchronize()
    idx = d_idx[:m].cpu().numpy()
    check(name, idx, st)
    assert np.all(d_idx[m:].cpu().numpy() == -1)         # nothing written past the count
    assert np.array_equal(o_rec[:m].cpu().numpy().view(np.uint32), rec[idx].view(np.uint32))
    assert np.array_equal(o_nrm[:m].cpu().numpy().view(np.uint32), nrm[idx].view(np.uint32))
    assert not o_rec[m:].any().item() and not o_nrm[m:].any().item()
