// rsm_ply.cpp -- the four binary little-endian PLY writers of include/rsm.h.  Host only.
#include "../../include/rsm.h"

#include <stdio.h>

// The frame of every file: open, the header (the vertex element with `vertex_props` behind x y z; the face element when nf >= 0),
// the vertex records (`vertices`) and the faces, ferror, close.
template <typename Vertices>
static int write_ply_file(const char *path, int64_t nv, const char *vertex_props, const int32_t *faces, int64_t nf, Vertices vertices) {
    FILE *fp = fopen(path, "wb");
    if (!fp) return RSM_E_INVALID;
    fprintf(fp, "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s", (int)nv, vertex_props);
    if (nf >= 0) fprintf(fp, "element face %d\nproperty list uchar int vertex_indices\n", (int)nf);
    fprintf(fp, "end_header\n");
    vertices(fp);
    const unsigned char three = 3;
    for (int64_t f = 0; f < nf; f++) {
        fwrite(&three, 1, 1, fp);
        fwrite(faces + 3 * f, sizeof(int32_t), 3, fp);
    }
    const int ok = ferror(fp) == 0;
    fclose(fp);
    return ok ? RSM_OK : RSM_E_INVALID;
}
static const char *const kBgr = "property uchar blue\nproperty uchar green\nproperty uchar red\n";
static const char *const kRgb = "property uchar red\nproperty uchar green\nproperty uchar blue\n";
static bool mesh_args_ok(const char *path, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf) {
    return path && nv >= 0 && nf >= 0 && nv <= (int64_t)INT32_MAX && nf <= (int64_t)INT32_MAX && (nv == 0 || xyz) && (nf == 0 || faces);
}

// ---- the cloud (CStereoMatching.cpp:723-729, 754-756) ----------------------------------------------
extern "C" int rsm_write_ply(const char *path, const double *xyz, const uint8_t *bgr, int64_t n) {
    if (!path || n < 0 || (n > 0 && (!xyz || !bgr))) return RSM_E_INVALID;
    return write_ply_file(path, n, kBgr, nullptr, -1, [&](FILE *fp) {
        for (int64_t i = 0; i < n; i++) {
            const float p[3] = {(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]}; // convertTo CV_32F, .cpp:754
            fwrite(p, sizeof(float), 3, fp);
            fwrite(bgr + 3 * i, 1, 3, fp);
        }
    });
}

// the same file from the 16-byte records (float xyz + BGR are exactly a PLY vertex of this header)
extern "C" int rsm_write_ply16(const char *path, const rsm_point16 *points, int64_t n) {
    if (!path || n < 0 || (n > 0 && !points)) return RSM_E_INVALID;
    return write_ply_file(path, n, kBgr, nullptr, -1, [&](FILE *fp) {
        for (int64_t i = 0; i < n; i++) fwrite(&points[i], 1, 15, fp); // x, y, z, b, g, r (the pad byte stays behind)
    });
}

// ---- the mesh: what MeshLab and TextureStitcher read ---------------------------------------------------
extern "C" int rsm_write_ply_mesh(const char *path, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf) {
    if (!mesh_args_ok(path, xyz, nv, faces, nf)) return RSM_E_INVALID;
    return write_ply_file(path, nv, "", faces, nf, [&](FILE *fp) {
        if (nv > 0) fwrite(xyz, sizeof(float), 3 * (size_t)nv, fp);
    });
}

// the coloured mesh as MyPlyIo writes it (my_ply_interface.cpp:35-50): vertex x y z red green blue, face vertex_indices
extern "C" int rsm_write_ply_mesh_color(const char *path, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const uint8_t *rgb) {
    if (!mesh_args_ok(path, xyz, nv, faces, nf) || (nv > 0 && !rgb)) return RSM_E_INVALID;
    return write_ply_file(path, nv, kRgb, faces, nf, [&](FILE *fp) {
        for (int64_t v = 0; v < nv; v++) {
            fwrite(xyz + 3 * v, sizeof(float), 3, fp);
            fwrite(rgb + 3 * v, 1, 3, fp);
        }
    });
}
