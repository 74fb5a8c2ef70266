"""The MLS step's restatement (tests/mls_restatement.py) on shapes whose answer is known, and the new C ABI's surface
(names, struct layout, the PLY writer) -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mls_restatement import mls, mls_cloud, unit_orthogonal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsm.h")


def tilted_plane(n=3000, seed=0):
    rng = np.random.default_rng(seed)
    uv = rng.random((n, 2)) * 40.0 - 20.0
    nrm = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    e1 = np.cross(nrm, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    xyz = (np.array([5.0, -3.0, 100.0]) + uv[:, :1] * e1 + uv[:, 1:] * e2).astype(np.float32)
    return xyz, nrm


@pytest.mark.parametrize("order", [0, 1, 2])
def test_points_of_a_plane_stay_on_it_with_its_normal(order):
    xyz, nrm = tilted_plane()
    out, n, idx = mls_cloud(xyz, 2.5, order)
    assert len(idx) == len(xyz)                             # every point of a dense plane has neighbours
    off = (out.astype(np.float64) - np.array([5.0, -3.0, 100.0])) @ nrm
    assert np.abs(off).max() < 1e-4                         # (float32 input: ~1e-5 of rounding across the patch)
    cos = np.abs(n[:, :3].astype(np.float64) @ nrm)
    assert cos.min() > 1.0 - 1e-6
    assert np.abs(n[:, 3]).max() < 1e-6                     # no curvature


def test_order_2_fits_the_paraboloid_apex():
    rng = np.random.default_rng(3)
    uv = rng.random((4000, 2)) * 8.0 - 4.0
    uv[0] = 0.0                                             # the apex itself
    z = 0.05 * uv[:, 0] ** 2 + 0.12 * uv[:, 1] ** 2
    xyz = np.c_[uv, z].astype(np.float32)
    e, x, n = mls(xyz, 1.5, (1, 2), queries=[0])[2]
    assert e[0]
    assert np.allclose(n[0, :3] * np.sign(n[0, 2]), [0.0, 0.0, 1.0], atol=1e-4)
    assert abs(x[0, 2]) < 1e-4
    # order 1 (a plane fit by weighted least squares) does not follow the curvature at the apex: its point lifts
    e1, x1, _ = mls(xyz, 1.5, (1,), queries=[0])[1]
    assert e1[0] and x1[0, 2] > 1e-3


def test_unit_orthogonal_follows_eigens_rule():
    n = np.array([[0.0, 0.0, 1.0], [1e-14, 0.0, -1.0], [0.0, 2e-12, 1.0], [0.6, 0.0, 0.8], [0.0, 0.6, -0.8], [1.0, 0.0, 0.0]])
    n /= np.linalg.norm(n, axis=1)[:, None]
    v = unit_orthogonal(n)
    # |x| or |y| above 1e-12 |z|: (-y, x, 0) / |(x, y)|; otherwise (0, -z, y) / |(y, z)|
    assert np.allclose(v[0], [0.0, -1.0, 0.0]) and np.allclose(v[1], [0.0, 1.0, 0.0])
    assert np.allclose(v[2], [-1.0, 0.0, 0.0]) and np.allclose(v[3], [0.0, 1.0, 0.0])
    assert np.allclose(v[4], [-1.0, 0.0, 0.0]) and np.allclose(v[5], [0.0, 1.0, 0.0])
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0) and np.allclose(np.einsum("ij,ij->i", v, n), 0.0)


def test_sparse_and_nonfinite_points_emit_nothing():
    xyz, _ = tilted_plane(2000, 1)
    xyz[:2] = [[500.0, 500.0, 500.0], [500.5, 500.0, 500.0]]    # a pair: 2 neighbours each
    xyz[2] = [-500.0, 0.0, 0.0]                                  # alone
    xyz[3:6] = [[np.nan, 0.0, 100.0], [np.inf, 1.0, 2.0], [0.0, 0.0, -np.inf]]
    for order in (0, 1, 2):
        _, _, idx = mls_cloud(xyz, 2.5, order)
        assert not set(range(6)) & set(idx.tolist())
        assert len(idx) == len(xyz) - 6


def test_the_flip_follows_the_reference_normals():
    xyz, nrm = tilted_plane(1500, 2)
    ref = np.zeros((len(xyz), 4), np.float32)
    ref[:, :3] = nrm
    ref[::2, :3] = -nrm
    ref[5] = np.nan                                              # a NaN reference never flips
    out0, n0, idx0 = mls_cloud(xyz, 2.5, 1)
    out, n, idx = mls_cloud(xyz, 2.5, 1, ref)
    assert np.array_equal(idx, idx0) and np.array_equal(out, out0)
    dots = np.einsum("ij,ij->i", n[:, :3], ref[idx, :3])
    ok = np.isfinite(ref[idx, 0])
    assert np.all(dots[ok] >= 0)
    k = int(np.nonzero(idx == 5)[0][0])
    assert np.array_equal(n[k], n0[k])


def declared():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(rsm_[a-z0-9_]+)\s*\(", txt))


def test_the_mls_entry_points_are_declared_bound_and_exported():
    from reconstruction_amd import _lib
    names = {"rsm_mls_cloud", "rsm_mls_cloud_device"}
    assert names <= set(_lib.EXPORTS) and names <= declared()
    _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert names <= set(re.findall(r" T (rsm_[a-z0-9_]+)", out))


def test_mls_params_layout_as_gcc_sees_it(tmp_path):
    from reconstruction_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsm.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu\\n", sizeof(rsm_mls_params), offsetof(rsm_mls_params, search_radius), '
                   'offsetof(rsm_mls_params, polynomial_order));\nreturn 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.MlsParams), _lib.MlsParams.search_radius.offset, _lib.MlsParams.polynomial_order.offset]


def test_write_ply_pointnormal_round_trips(tmp_path):
    from reconstruction_amd import write_ply_pointnormal
    rng = np.random.default_rng(5)
    xyz = rng.normal(size=(37, 3)).astype(np.float32)
    nrm = rng.normal(size=(37, 4)).astype(np.float32)
    nrm[3] = np.nan
    p = tmp_path / "bigcloud.ply"
    write_ply_pointnormal(p, xyz, nrm)
    hdr, body = p.read_bytes().split(b"end_header\n", 1)
    props = [l.split()[-1] for l in hdr.decode().splitlines() if l.startswith("property float")]
    assert hdr.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 37\n")
    assert props == ["x", "y", "z", "normal_x", "normal_y", "normal_z", "curvature"]
    rec = np.frombuffer(body, "<f4").reshape(-1, 7)
    assert np.array_equal(rec[:, :3], xyz) and np.array_equal(rec[:, 3:], nrm, equal_nan=True)
