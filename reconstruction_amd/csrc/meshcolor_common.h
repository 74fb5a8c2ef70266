// meshcolor_common.h -- what the colouring (k_meshcolor.hip) and the seam levelling (k_meshstitch.hip) share: a view as the kernels see it,
// texture_color's pixel of a point, and the colouring with everything the levelling goes on from (the views and the corner lists on the
// device, in the caller's scratch).
#pragma once

#include "mesh_common.h"
#include "project_common.h"

// one view: R / T as float (cv2eigen of P's columns, as k_dedup), the centre in fp64, the images on the device
struct McView {
    float R[9], T[3];
    double C[3];
    int W, H;
    const uint8_t *img, *mask; // BGR, stride 3 W; mask may be NULL: all 255
    uint32_t *wbuf;            // W x H
};

__device__ __forceinline__ void mcol_q(const McView &c, float px, float py, float pz, float *q0, float *q1, float *q2) {
    *q0 = dd_dot3(c.R[0], c.R[1], c.R[2], px, py, pz) + c.T[0];
    *q1 = dd_dot3(c.R[3], c.R[4], c.R[5], px, py, pz) + c.T[1];
    *q2 = dd_dot3(c.R[6], c.R[7], c.R[8], px, py, pz) + c.T[2];
}

// the texture_color pixel of a projected point; false where texture_color answers (127, 127, 127)
__device__ __forceinline__ bool mcol_pixel(float q0, float q1, float q2, int W, int H, size_t *pix) {
    long long x, y;
    if (!dd_round(q0 / q2, &x) || !dd_round(q1 / q2, &y)) return false;
    if (x < 0 || x >= W || y < 0 || y >= H) return false;
    *pix = (size_t)y * (size_t)W + (size_t)x;
    return true;
}

struct rsm_dedup_view;
struct rsm_mesh_color_params;
// The V = 2 n_pairs views in scans.txt's order on the device, their host images uploaded into M (with_wbuf: and a depth buffer each).
// RSM_E_INVALID comes with *invalid = 3 (a singular P).  The uploads are only enqueued: the caller waits for `st` before the host images go.
int mesh_views_device(DevMem &M, const rsm_dedup_view *views, int n_pairs, bool with_wbuf, std::vector<McView> *hv, McView **d_views, int *invalid, hipStream_t st);
// mesh_color_device (rsm_dev.h) with its scratch in the caller's M, so that what it built outlives it: d_vis (may be NULL) receives per
// vertex the mask of the views that see it (bit v = view v; V <= 64 then), scene the views and the corner lists.  nv = 0: nothing is built.
struct McScene {
    const McView *d_views = nullptr;
    int V = 0;
    const uint32_t *row = nullptr, *corner = nullptr;
};
int mesh_color_scene_device(DevMem &M, const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                            const rsm_mesh_color_params *p, long long big_box, uint8_t *d_rgb, int32_t *d_best, unsigned long long *d_vis, double *stats,
                            int *invalid, McScene *scene, hipStream_t st);
