"""The four PLY writers of the C ABI, byte for byte (host code: no GPU).

Each file is compared whole with bytes assembled here: the header text of DESIGN.md 9 f4 / f7 / f9 (binary little-endian, the
reference's property order) and numpy's own bytes of the payload.  A tiny fixed input and the empty one per writer."""
import ctypes as C

import numpy as np
import pytest

from reconstruction_amd import _lib

CLOUD_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar blue\nproperty uchar green\nproperty uchar red\nend_header\n")
MESH_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
               "%selement face %d\nproperty list uchar int vertex_indices\nend_header\n")
RGB_PROPS = "property uchar red\nproperty uchar green\nproperty uchar blue\n"

XYZ64 = np.array([[0.1, -2.5, 3.0], [1e-3, 7.0, -0.0], [123456.789, -1e10, 5e-8]], np.float64)   # not float32 numbers: the cast shows
BGR = np.array([[0, 1, 2], [255, 128, 7], [9, 8, 250]], np.uint8)
VERTS = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, -0.25], [1.5, 1, 1e-3]], np.float32)
FACES = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
RGB = np.array([[10, 20, 30], [0, 255, 1], [200, 100, 50], [7, 7, 7]], np.uint8)


def _p(a):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(None)


def _written(tmp_path, name, *args):
    path = tmp_path / "out.ply"
    st = getattr(_lib.load(), name)(C.c_char_p(str(path).encode()), *args)
    assert st == _lib.RSM_OK, (name, st)
    return path.read_bytes()


def _face_bytes(faces):
    rec = np.zeros(len(faces), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))   # packed: uchar 3 + three int32
    rec["n"] = 3
    rec["v"] = faces
    assert rec.dtype.itemsize == 13
    return rec.tobytes()


@pytest.mark.parametrize("n", [3, 0])
def test_write_ply(tmp_path, n):
    xyz, bgr = np.ascontiguousarray(XYZ64[:n]), np.ascontiguousarray(BGR[:n])
    got = _written(tmp_path, "rsm_write_ply", _p(xyz), _p(bgr), C.c_int64(n))
    body = b"".join(xyz[i].astype("<f4").tobytes() + bgr[i].tobytes() for i in range(n))
    assert got == (CLOUD_HEADER % n).encode() + body


@pytest.mark.parametrize("n", [3, 0])
def test_write_ply16(tmp_path, n):
    rec = np.zeros(n, np.dtype([("xyz", "<f4", (3,)), ("bgr", "u1", (3,)), ("pad", "u1")]))
    assert rec.dtype.itemsize == 16
    rec["xyz"] = XYZ64[:n]
    rec["bgr"] = BGR[:n]
    rec["pad"] = 0xEE   # the 16th byte of a record stays behind
    got = _written(tmp_path, "rsm_write_ply16", _p(rec), C.c_int64(n))
    body = b"".join(rec[i].tobytes()[:15] for i in range(n))
    assert got == (CLOUD_HEADER % n).encode() + body
    assert len(got) == len(CLOUD_HEADER % n) + 15 * n


@pytest.mark.parametrize("nv,nf", [(4, 2), (0, 0)])
def test_write_ply_mesh(tmp_path, nv, nf):
    v, f = np.ascontiguousarray(VERTS[:nv]), np.ascontiguousarray(FACES[:nf])
    got = _written(tmp_path, "rsm_write_ply_mesh", _p(v), C.c_int64(nv), _p(f), C.c_int64(nf))
    assert got == (MESH_HEADER % (nv, "", nf)).encode() + v.tobytes() + _face_bytes(f)


@pytest.mark.parametrize("nv,nf", [(4, 2), (0, 0)])
def test_write_ply_mesh_color(tmp_path, nv, nf):
    v, f, c = np.ascontiguousarray(VERTS[:nv]), np.ascontiguousarray(FACES[:nf]), np.ascontiguousarray(RGB[:nv])
    got = _written(tmp_path, "rsm_write_ply_mesh_color", _p(v), C.c_int64(nv), _p(f), C.c_int64(nf), _p(c))
    body = b"".join(v[i].tobytes() + c[i].tobytes() for i in range(nv))
    assert got == (MESH_HEADER % (nv, RGB_PROPS, nf)).encode() + body + _face_bytes(f)
