// rsm_mesh.hip -- the mesh back end's host side after the surface itself (rsm_poisson.hip): the mesh-to-mesh stages (smoothing and clean-up, the
// density trim, the closing of holes, the decimation, the subdivision) and the colours from the rig's views with their seams levelled and their gaps
// filled (k_meshclean.hip, k_meshtrim.hip, k_meshclose.hip, k_meshdecimate.hip, k_meshsubdivide.hip, k_meshcolor.hip, k_meshstitch.hip, k_meshfill.hip).
#include "rsm_ctx.h"

#include <cmath>
#include <string.h>

// ---- the mesh-to-mesh stages: clean, trim, close_holes, decimate, subdivide (how the back end's units are laid out) -------------------------
static int mesh_counts_ok(rsm_ctx *c, const char *who, int64_t nv, int64_t nf) { // who: "mesh_clean" / "mesh_trim" / "mesh_color" ...
    if (nv < 0 || nv > (int64_t)INT32_MAX) return set_err(c, RSM_E_INVALID, "%s: nv %lld outside 0..INT32_MAX", who, (long long)nv);
    if (nf < 0 || 3 * nf >= ((int64_t)1 << 31)) return set_err(c, RSM_E_INVALID, "%s: nf %lld negative or 3 nf >= 2^31", who, (long long)nf);
    return RSM_OK;
}
static int no_check() { return RSM_OK; }
// the counts, what the stage checks next (trim's n), then the pointers
template <class Extra>
static int mesh_in_ok(rsm_ctx *c, const char *who, int64_t nv, int64_t nf, const float *xyz, const int32_t *faces, const int64_t *n_vertices, const int64_t *n_faces,
                      Extra extra_ok) {
    int s = mesh_counts_ok(c, who, nv, nf);
    if (s != RSM_OK || (s = extra_ok()) != RSM_OK) return s;
    if (!n_vertices || !n_faces || (nv > 0 && !xyz) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "%s: a NULL pointer", who);
    return RSM_OK;
}
// invalid: mesh_validate_device's 1 / 2
static int mesh_fail(rsm_ctx *c, const char *who, int s, int invalid) {
    if (s == RSM_E_INVALID && invalid >= MESH_INVALID_TOO_LARGE)
        return set_err(c, s, "%s: the result of iteration %d would be too large (vertices above INT32_MAX or 3 nf >= 2^31)", who, invalid - MESH_INVALID_TOO_LARGE + 1);
    if (s == RSM_E_INVALID) return set_err(c, s, invalid == 1 ? "%s: a face index outside [0, nv)" : "%s: a coordinate that is not finite", who);
    if (s == RSM_E_NOMEM) return set_err(c, s, "%s: no device memory", who);
    return set_err(c, s, "%s: failed%s", who, hip_tail(s).c_str());
}

// where a stage's mesh comes from: host arrays, device buffers, or the context's last mesh (no arrays then: its counts need no check)
enum MeshFrom { MESH_HOST, MESH_DEVICE, MESH_LAST };
struct MeshIn {
    MeshFrom from;
    const float *xyz = nullptr;
    int64_t nv = 0;
    const int32_t *faces = nullptr;
    int64_t nf = 0;
};
// One stage `who`, the same from every source.  params_ok() / extra_ok(): the stage's checks in front of and behind the counts;
// run(d_v, nv, d_f, nf, &c->pmesh, stats, &invalid): its *_device function, whose result replaces the context's last mesh (d_v / d_f may be
// that mesh's own buffers).  A refused or failed call leaves mesh and colours as they were.  The two halves are there for the trim, which
// uploads its samples between them.
template <class ParamsOk, class ExtraOk>
static int mesh_stage_check(rsm_ctx *c, const char *who, const MeshIn &in, ParamsOk params_ok, ExtraOk extra_ok, const int64_t *n_vertices, const int64_t *n_faces) {
    if (!c) return RSM_E_INVALID;
    const int s = params_ok();
    if (s != RSM_OK) return s;
    return mesh_in_ok(c, who, in.nv, in.nf, in.xyz, in.faces, n_vertices, n_faces, extra_ok);
}
template <class Run>
static int mesh_stage_run(rsm_ctx *c, const char *who, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, Run run, int64_t *n_vertices, int64_t *n_faces,
                          double *stats) {
    int invalid = 0;
    const int s = run(d_xyz, nv, d_faces, nf, &c->pmesh, stats, &invalid);
    if (s != RSM_OK) return mesh_fail(c, who, s, invalid);
    mesh_replaced(c);
    *n_vertices = c->pmesh.nv;
    *n_faces = c->pmesh.nf;
    return RSM_OK;
}
template <class ParamsOk, class ExtraOk, class Run>
static int mesh_stage(rsm_ctx *c, const char *who, const MeshIn &in, ParamsOk params_ok, ExtraOk extra_ok, Run run, int64_t *n_vertices, int64_t *n_faces, double *stats) {
    int s = mesh_stage_check(c, who, in, params_ok, extra_ok, n_vertices, n_faces);
    if (s != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if (in.from == MESH_LAST) return mesh_stage_run(c, who, c->pmesh.d_v, c->pmesh.nv, c->pmesh.d_f, c->pmesh.nf, run, n_vertices, n_faces, stats);
    if (in.from == MESH_DEVICE) return mesh_stage_run(c, who, in.xyz, in.nv, in.faces, in.nf, run, n_vertices, n_faces, stats);
    Tmp T(c);
    float *dv = T.up(in.xyz, 3 * (size_t)in.nv);
    int32_t *df = T.up(in.faces, 3 * (size_t)in.nf);
    if (!dv || !df) return set_err(c, RSM_E_NOMEM, "%s: no device memory for %lld vertices, %lld faces", who, (long long)in.nv, (long long)in.nf);
    if ((s = finish(c, T)) != RSM_OK) return s;
    return mesh_stage_run(c, who, dv, in.nv, df, in.nf, run, n_vertices, n_faces, stats);
}
// ... of a stage whose *_device function takes the caller's params as they are (every one but the trim)
template <class P>
static int mesh_stage_p(rsm_ctx *c, const char *who, const MeshIn &in, const P *p, int (*params_ok)(rsm_ctx *, const P *),
                        int (*device)(const float *, int64_t, const int32_t *, int64_t, const P *, PoissonMesh *, double *, int *, hipStream_t), int64_t *n_vertices,
                        int64_t *n_faces, double *stats) {
    return mesh_stage(
        c, who, in, [&] { return params_ok(c, p); }, no_check,
        [&](const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, PoissonMesh *out, double *st, int *invalid) {
            return device(d_v, nv, d_f, nf, p, out, st, invalid, c->stream);
        },
        n_vertices, n_faces, stats);
}

// ---- smoothing and clean-up of the surface (k_meshclean.hip) ------------------------------------------------------------
static int meshclean_params_ok(rsm_ctx *c, const rsm_mesh_clean_params *p) {
    if (!p) return set_err(c, RSM_E_INVALID, "mesh_clean: params is NULL");
    if (p->smooth_steps < 0) return set_err(c, RSM_E_INVALID, "mesh_clean: smooth_steps %d < 0", p->smooth_steps);
    if (p->cotangent != 0 && p->cotangent != 1) return set_err(c, RSM_E_INVALID, "mesh_clean: cotangent %d not 0 or 1", p->cotangent);
    if (p->boundary != 0 && p->boundary != 1) return set_err(c, RSM_E_INVALID, "mesh_clean: boundary %d not 0 or 1", p->boundary);
    if (!std::isfinite(p->min_piece) || p->min_piece < 0.0) return set_err(c, RSM_E_INVALID, "mesh_clean: min_piece %g negative or not finite", p->min_piece);
    if (p->min_piece_relative != 0 && p->min_piece_relative != 1)
        return set_err(c, RSM_E_INVALID, "mesh_clean: min_piece_relative %d not 0 or 1", p->min_piece_relative);
    if (p->flags & ~(RSM_MESH_CLEAN_DUPLICATES | RSM_MESH_CLEAN_ZERO_AREA | RSM_MESH_CLEAN_NONMANIFOLD))
        return set_err(c, RSM_E_INVALID, "mesh_clean: flags 0x%x has an unknown bit", p->flags);
    return RSM_OK;
}
extern "C" int rsm_mesh_clean_device(rsm_ctx *c, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_mesh_clean_params *p,
                                     int64_t *n_vertices, int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_clean", MeshIn{MESH_DEVICE, d_xyz, nv, d_faces, nf}, p, meshclean_params_ok, mesh_clean_device, n_vertices, n_faces, stats);
}
extern "C" int rsm_mesh_clean(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_clean_params *p, int64_t *n_vertices,
                              int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_clean", MeshIn{MESH_HOST, xyz, nv, faces, nf}, p, meshclean_params_ok, mesh_clean_device, n_vertices, n_faces, stats);
}
extern "C" int rsm_mesh_clean_last(rsm_ctx *c, const rsm_mesh_clean_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_clean", MeshIn{MESH_LAST}, p, meshclean_params_ok, mesh_clean_device, n_vertices, n_faces, stats);
}

extern "C" int rsm_stage_mesh_smooth(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, int steps, int cotangent, int boundary,
                                     float *out_xyz, int64_t *n_border) {
    if (!c) return RSM_E_INVALID;
    const rsm_mesh_clean_params p{steps, cotangent, boundary, 0.0, 0, 0u};
    int s = meshclean_params_ok(c, &p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_clean", nv, nf)) != RSM_OK) return s;
    if ((nv > 0 && (!xyz || !out_xyz)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_clean: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv), *dout = T.alloc<float>(3 * (size_t)nv);
    int32_t *df = T.up(faces, 3 * (size_t)nf);
    if (!dv || !dout || !df) return set_err(c, RSM_E_NOMEM, "mesh_clean: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    int64_t nb = 0;
    if ((s = mesh_smooth_device(dv, nv, df, nf, steps, cotangent, boundary, dout, &nb, &invalid, c->stream)) != RSM_OK) return mesh_fail(c, "mesh_clean", s, invalid);
    T.later(out_xyz, dout, 3 * (size_t)nv);
    if ((s = finish(c, T)) != RSM_OK) return s;
    if (n_border) *n_border = nb;
    return RSM_OK;
}

extern "C" int rsm_stage_mesh_components(rsm_ctx *c, const int32_t *faces, int64_t nv, int64_t nf, int32_t *labels, int64_t *n_components) {
    if (!c) return RSM_E_INVALID;
    int s = mesh_counts_ok(c, "mesh_clean", nv, nf);
    if (s != RSM_OK) return s;
    if (!n_components || (nf > 0 && (!faces || !labels))) return set_err(c, RSM_E_INVALID, "mesh_clean: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *dl = T.alloc<int32_t>((size_t)nf);
    if (!df || !dl) return set_err(c, RSM_E_NOMEM, "mesh_clean: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_components_device(df, nv, nf, dl, n_components, &invalid, c->stream)) != RSM_OK) return mesh_fail(c, "mesh_clean", s, invalid);
    T.later(labels, dl, (size_t)nf);
    return finish(c, T);
}

// ---- the density trim of the surface (k_meshtrim.hip) -------------------------------------------------------------------
static int meshtrim_params_ok(rsm_ctx *c, const rsm_mesh_trim_params *p) {
    if (!p) return set_err(c, RSM_E_INVALID, "mesh_trim: params is NULL");
    if (p->depth < 5 || p->depth > 9) return set_err(c, RSM_E_INVALID, "mesh_trim: depth %d outside 5..9", p->depth);
    if (!std::isfinite(p->scale) || p->scale < 1.0) return set_err(c, RSM_E_INVALID, "mesh_trim: scale %g not finite or < 1", p->scale);
    if (p->kernel_depth != 0 && (p->kernel_depth < 3 || p->kernel_depth > p->depth))
        return set_err(c, RSM_E_INVALID, "mesh_trim: kernel_depth %d neither 0 nor in 3..depth (%d)", p->kernel_depth, p->depth);
    if (!std::isfinite(p->samples_per_node) || !(p->samples_per_node > 0.0))
        return set_err(c, RSM_E_INVALID, "mesh_trim: samples_per_node %g not finite or not > 0", p->samples_per_node);
    if (p->smooth_steps < 0) return set_err(c, RSM_E_INVALID, "mesh_trim: smooth_steps %d < 0", p->smooth_steps);
    if (!std::isfinite(p->trim)) return set_err(c, RSM_E_INVALID, "mesh_trim: trim %g not finite", p->trim);
    if (!(p->island_ratio >= 0.0 && p->island_ratio < 1.0)) return set_err(c, RSM_E_INVALID, "mesh_trim: island_ratio %g not in [0, 1)", p->island_ratio);
    return RSM_OK;
}
static int meshtrim_n_ok(rsm_ctx *c, int64_t n) {
    if (n < 0 || n > (int64_t)INT32_MAX) return set_err(c, RSM_E_INVALID, "mesh_trim: n %lld outside 0..INT32_MAX", (long long)n);
    return RSM_OK;
}
static int meshtrim_values_ok(rsm_ctx *c, const double *values, int64_t nv) {
    for (int64_t i = 0; i < nv; i++)
        if (!std::isfinite(values[i])) return set_err(c, RSM_E_INVALID, "mesh_trim: values[%lld] is not finite", (long long)i);
    return RSM_OK;
}
// the samples a trim is given: checked between the counts and the pointers; the entries with host samples upload them themselves
struct TrimSamples {
    const float *xyz, *normals4;
    int64_t n;
};
static int meshtrim_samples_ok(rsm_ctx *c, const TrimSamples &S) {
    const int s = meshtrim_n_ok(c, S.n);
    if (s != RSM_OK) return s;
    if (S.n > 0 && !S.xyz) return set_err(c, RSM_E_INVALID, "mesh_trim: a NULL pointer");
    return RSM_OK;
}
static auto meshtrim_run(rsm_ctx *c, const TrimSamples &D, const rsm_mesh_trim_params *p) { // D: on the device
    return [=](const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, PoissonMesh *out, double *st, int *invalid) {
        return mesh_trim_device(d_v, nv, d_f, nf, D.xyz, D.normals4, D.n, p, out, st, invalid, c->stream);
    };
}

extern "C" int rsm_mesh_trim_device(rsm_ctx *c, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const float *d_samples_xyz,
                                    const float *d_samples_normals4, int64_t n, const rsm_mesh_trim_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats) {
    const TrimSamples D{d_samples_xyz, d_samples_normals4, n};
    return mesh_stage(
        c, "mesh_trim", MeshIn{MESH_DEVICE, d_xyz, nv, d_faces, nf}, [&] { return meshtrim_params_ok(c, p); }, [&] { return meshtrim_samples_ok(c, D); },
        meshtrim_run(c, D, p), n_vertices, n_faces, stats);
}

extern "C" int rsm_mesh_trim(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const float *samples_xyz, const float *samples_normals4,
                             int64_t n, const rsm_mesh_trim_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats) {
    const TrimSamples S{samples_xyz, samples_normals4, n};
    int s = mesh_stage_check(
        c, "mesh_trim", MeshIn{MESH_HOST, xyz, nv, faces, nf}, [&] { return meshtrim_params_ok(c, p); }, [&] { return meshtrim_samples_ok(c, S); }, n_vertices, n_faces);
    if (s != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv), *dx = T.up(samples_xyz, 3 * (size_t)n), *dn = samples_normals4 ? T.up(samples_normals4, 4 * (size_t)n) : nullptr;
    int32_t *df = T.up(faces, 3 * (size_t)nf);
    if (!dv || !dx || !df || (samples_normals4 && !dn))
        return set_err(c, RSM_E_NOMEM, "mesh_trim: no device memory for %lld vertices, %lld faces, %lld samples", (long long)nv, (long long)nf, (long long)n);
    if ((s = finish(c, T)) != RSM_OK) return s;
    return mesh_stage_run(c, "mesh_trim", dv, nv, df, nf, meshtrim_run(c, TrimSamples{dx, dn, n}, p), n_vertices, n_faces, stats);
}

extern "C" int rsm_mesh_trim_last(rsm_ctx *c, const float *samples_xyz, const float *samples_normals4, int64_t n, const rsm_mesh_trim_params *p, int64_t *n_vertices,
                                  int64_t *n_faces, double *stats) {
    const TrimSamples S{samples_xyz, samples_normals4, n};
    int s = mesh_stage_check(c, "mesh_trim", MeshIn{MESH_LAST}, [&] { return meshtrim_params_ok(c, p); }, [&] { return meshtrim_samples_ok(c, S); }, n_vertices, n_faces);
    if (s != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dx = T.up(samples_xyz, 3 * (size_t)n), *dn = samples_normals4 ? T.up(samples_normals4, 4 * (size_t)n) : nullptr;
    if (!dx || (samples_normals4 && !dn)) return set_err(c, RSM_E_NOMEM, "mesh_trim: no device memory for %lld samples", (long long)n);
    if ((s = finish(c, T)) != RSM_OK) return s;
    return mesh_stage_run(c, "mesh_trim", c->pmesh.d_v, c->pmesh.nv, c->pmesh.d_f, c->pmesh.nf, meshtrim_run(c, TrimSamples{dx, dn, n}, p), n_vertices, n_faces, stats);
}

extern "C" int rsm_stage_mesh_density(rsm_ctx *c, const float *samples_xyz, const float *samples_normals4, int64_t n, const rsm_mesh_trim_params *p, const float *xyz,
                                      int64_t nv, double *rho, double *value, int64_t counts[2]) {
    if (!c) return RSM_E_INVALID;
    int s = meshtrim_params_ok(c, p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_trim", nv, 0)) != RSM_OK || (s = meshtrim_n_ok(c, n)) != RSM_OK) return s;
    if (!counts || (nv > 0 && (!xyz || !rho || !value)) || (n > 0 && !samples_xyz)) return set_err(c, RSM_E_INVALID, "mesh_trim: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv), *dx = T.up(samples_xyz, 3 * (size_t)n), *dn = samples_normals4 ? T.up(samples_normals4, 4 * (size_t)n) : nullptr;
    double *dr = T.alloc<double>((size_t)nv), *da = T.alloc<double>((size_t)nv);
    if (!dv || !dx || !dr || !da || (samples_normals4 && !dn)) return set_err(c, RSM_E_NOMEM, "mesh_trim: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    double hk = 0.0;
    const int kd = p->kernel_depth ? p->kernel_depth : p->depth - 2;
    if ((s = mesh_density_device(dx, dn, n, p->depth, p->scale, kd, p->samples_per_node, dv, nv, dr, da, counts, &hk, &invalid, c->stream)) != RSM_OK)
        return mesh_fail(c, "mesh_trim", s, invalid);
    T.later(rho, dr, (size_t)nv).later(value, da, (size_t)nv);
    return finish(c, T);
}

extern "C" int rsm_stage_mesh_value_smooth(rsm_ctx *c, const int32_t *faces, int64_t nv, int64_t nf, const double *values, int steps, double *out_values) {
    if (!c) return RSM_E_INVALID;
    int s = mesh_counts_ok(c, "mesh_trim", nv, nf);
    if (s != RSM_OK) return s;
    if (steps < 0) return set_err(c, RSM_E_INVALID, "mesh_trim: smooth_steps %d < 0", steps);
    if ((nv > 0 && (!values || !out_values)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_trim: a NULL pointer");
    if ((s = meshtrim_values_ok(c, values, nv)) != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    int32_t *df = T.up(faces, 3 * (size_t)nf);
    double *din = T.up(values, (size_t)nv), *dout = T.alloc<double>((size_t)nv);
    if (!df || !din || !dout) return set_err(c, RSM_E_NOMEM, "mesh_trim: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_value_smooth_device(df, nv, nf, din, steps, dout, &invalid, c->stream)) != RSM_OK) return mesh_fail(c, "mesh_trim", s, invalid);
    T.later(out_values, dout, (size_t)nv);
    return finish(c, T);
}

extern "C" int rsm_stage_mesh_split(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const double *values, double trim, double island_ratio,
                                    int64_t *n_vertices, int64_t *n_faces, double *stats, int32_t *src_face, int32_t *side, int32_t *label) {
    if (!c) return RSM_E_INVALID;
    const rsm_mesh_trim_params p{5, 1.0, 0, 1.0, 0, trim, island_ratio};
    int s = meshtrim_params_ok(c, &p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_trim", nv, nf)) != RSM_OK) return s;
    if (!n_vertices || !n_faces || (nv > 0 && (!xyz || !values)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_trim: a NULL pointer");
    if ((s = meshtrim_values_ok(c, values, nv)) != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *dsrc = T.alloc<int32_t>(3 * (size_t)nf), *dside = T.alloc<int32_t>(3 * (size_t)nf), *dlab = T.alloc<int32_t>(3 * (size_t)nf);
    double *dx = T.up(values, (size_t)nv);
    if (!dv || !df || !dsrc || !dside || !dlab || !dx) return set_err(c, RSM_E_NOMEM, "mesh_trim: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_split_device(dv, nv, df, nf, dx, trim, island_ratio, &c->pmesh, dsrc, dside, dlab, stats, &invalid, c->stream)) != RSM_OK)
        return mesh_fail(c, "mesh_trim", s, invalid);
    mesh_replaced(c);
    *n_vertices = c->pmesh.nv;
    *n_faces = c->pmesh.nf;
    const size_t m = (size_t)c->pmesh.nf;
    T.later(src_face, dsrc, m).later(side, dside, m).later(label, dlab, m);
    return finish(c, T);
}

// ---- the closing of the surface's small holes (k_meshclose.hip) ---------------------------------------------------------
static int meshclose_params_ok(rsm_ctx *c, const rsm_mesh_close_params *p) {
    if (!p) return set_err(c, RSM_E_INVALID, "mesh_close_holes: params is NULL");
    if (p->max_hole_size < 3 || p->max_hole_size > RSM_MESH_CLOSE_MAX_HOLE)
        return set_err(c, RSM_E_INVALID, "mesh_close_holes: max_hole_size %d outside 3..%d", p->max_hole_size, RSM_MESH_CLOSE_MAX_HOLE);
    return RSM_OK;
}
extern "C" int rsm_mesh_close_holes_device(rsm_ctx *c, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_mesh_close_params *p,
                                           int64_t *n_vertices, int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_close_holes", MeshIn{MESH_DEVICE, d_xyz, nv, d_faces, nf}, p, meshclose_params_ok, mesh_close_holes_device, n_vertices, n_faces, stats);
}
extern "C" int rsm_mesh_close_holes(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_close_params *p, int64_t *n_vertices,
                                    int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_close_holes", MeshIn{MESH_HOST, xyz, nv, faces, nf}, p, meshclose_params_ok, mesh_close_holes_device, n_vertices, n_faces, stats);
}
extern "C" int rsm_mesh_close_holes_last(rsm_ctx *c, const rsm_mesh_close_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_close_holes", MeshIn{MESH_LAST}, p, meshclose_params_ok, mesh_close_holes_device, n_vertices, n_faces, stats);
}

extern "C" int rsm_stage_mesh_border_loops(rsm_ctx *c, const int32_t *faces, int64_t nv, int64_t nf, int32_t *labels, int32_t *sizes, int64_t *n_components) {
    if (!c) return RSM_E_INVALID;
    int s = mesh_counts_ok(c, "mesh_close_holes", nv, nf);
    if (s != RSM_OK) return s;
    if (!n_components || (nf > 0 && (!faces || !labels || !sizes))) return set_err(c, RSM_E_INVALID, "mesh_close_holes: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *dl = T.alloc<int32_t>(3 * (size_t)nf), *ds = T.alloc<int32_t>(3 * (size_t)nf);
    if (!df || !dl || !ds) return set_err(c, RSM_E_NOMEM, "mesh_close_holes: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_border_loops_device(df, nv, nf, dl, ds, n_components, &invalid, c->stream)) != RSM_OK) return mesh_fail(c, "mesh_close_holes", s, invalid);
    T.later(labels, dl, 3 * (size_t)nf).later(sizes, ds, 3 * (size_t)nf);
    return finish(c, T);
}

extern "C" int rsm_stage_hole_triangulate(rsm_ctx *c, const float *ring_xyz, int L, const uint8_t *forbidden, double *weight, int32_t *triangles, int *n_triangles) {
    if (!c) return RSM_E_INVALID;
    if (L < 3 || L > RSM_MESH_CLOSE_MAX_HOLE) return set_err(c, RSM_E_INVALID, "mesh_close_holes: L %d outside 3..%d", L, RSM_MESH_CLOSE_MAX_HOLE);
    if (!ring_xyz || !weight || !triangles || !n_triangles) return set_err(c, RSM_E_INVALID, "mesh_close_holes: a NULL pointer");
    for (int i = 0; i < 3 * L; i++)
        if (!std::isfinite(ring_xyz[i])) return set_err(c, RSM_E_INVALID, "mesh_close_holes: a coordinate that is not finite");
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dr = T.up(ring_xyz, 3 * (size_t)L);
    uint8_t *dm = forbidden ? T.up(forbidden, (size_t)L * (size_t)L) : nullptr;
    int32_t *dt = T.alloc<int32_t>(3 * (size_t)(L - 2));
    if (!dr || !dt || (forbidden && !dm)) return set_err(c, RSM_E_NOMEM, "mesh_close_holes: no device memory");
    int s = finish(c, T);
    if (s != RSM_OK) return s;
    if ((s = hole_triangulate_device(dr, L, dm, weight, dt, n_triangles, c->stream)) != RSM_OK) return mesh_fail(c, "mesh_close_holes", s, 0);
    T.later(triangles, dt, 3 * (size_t)*n_triangles);
    return finish(c, T);
}

// ---- the decimation of the final mesh (k_meshdecimate.hip) ----------------------------------------------------------------
static int meshdecimate_params_ok(rsm_ctx *c, const rsm_mesh_decimate_params *p) {
    if (!p) return set_err(c, RSM_E_INVALID, "mesh_decimate: params is NULL");
    if (p->target_faces < 0) return set_err(c, RSM_E_INVALID, "mesh_decimate: target_faces %lld < 0", (long long)p->target_faces);
    if (!(p->target_fraction >= 0.0 && p->target_fraction <= 1.0)) return set_err(c, RSM_E_INVALID, "mesh_decimate: target_fraction %g outside [0, 1]", p->target_fraction);
    if (!(p->quality_thr >= 0.0 && p->quality_thr <= 1.0)) return set_err(c, RSM_E_INVALID, "mesh_decimate: quality_thr %g outside [0, 1]", p->quality_thr);
    if (!std::isfinite(p->boundary_weight) || !(p->boundary_weight > 0.0))
        return set_err(c, RSM_E_INVALID, "mesh_decimate: boundary_weight %g not finite or not positive", p->boundary_weight);
    if (!std::isfinite(p->min_error) || p->min_error < 0.0) return set_err(c, RSM_E_INVALID, "mesh_decimate: min_error %g negative or not finite", p->min_error);
    if (p->max_rounds < 1 || p->max_rounds > 1000000) return set_err(c, RSM_E_INVALID, "mesh_decimate: max_rounds %d outside 1..1000000", p->max_rounds);
    const int flag[4] = {p->preserve_boundary, p->preserve_normal, p->preserve_topology, p->optimal_placement};
    const char *name[4] = {"preserve_boundary", "preserve_normal", "preserve_topology", "optimal_placement"};
    for (int i = 0; i < 4; i++)
        if (flag[i] != 0 && flag[i] != 1) return set_err(c, RSM_E_INVALID, "mesh_decimate: %s %d not 0 or 1", name[i], flag[i]);
    return RSM_OK;
}
extern "C" int rsm_mesh_decimate_device(rsm_ctx *c, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_mesh_decimate_params *p,
                                        int64_t *n_vertices, int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_decimate", MeshIn{MESH_DEVICE, d_xyz, nv, d_faces, nf}, p, meshdecimate_params_ok, mesh_decimate_device, n_vertices, n_faces, stats);
}
extern "C" int rsm_mesh_decimate(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_decimate_params *p, int64_t *n_vertices,
                                 int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_decimate", MeshIn{MESH_HOST, xyz, nv, faces, nf}, p, meshdecimate_params_ok, mesh_decimate_device, n_vertices, n_faces, stats);
}
extern "C" int rsm_mesh_decimate_last(rsm_ctx *c, const rsm_mesh_decimate_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_decimate", MeshIn{MESH_LAST}, p, meshdecimate_params_ok, mesh_decimate_device, n_vertices, n_faces, stats);
}

extern "C" int rsm_stage_mesh_quadrics(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, double boundary_weight, double *out_q) {
    if (!c) return RSM_E_INVALID;
    int s = mesh_counts_ok(c, "mesh_decimate", nv, nf);
    if (s != RSM_OK) return s;
    if (!std::isfinite(boundary_weight) || !(boundary_weight > 0.0))
        return set_err(c, RSM_E_INVALID, "mesh_decimate: boundary_weight %g not finite or not positive", boundary_weight);
    if ((nv > 0 && (!xyz || !out_q)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_decimate: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv);
    int32_t *df = T.up(faces, 3 * (size_t)nf);
    double *dq = T.alloc<double>(10 * (size_t)nv);
    if (!dv || !df || !dq) return set_err(c, RSM_E_NOMEM, "mesh_decimate: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_quadrics_device(dv, nv, df, nf, boundary_weight, dq, &invalid, c->stream)) != RSM_OK) return mesh_fail(c, "mesh_decimate", s, invalid);
    T.later(out_q, dq, 10 * (size_t)nv);
    return finish(c, T);
}

extern "C" int rsm_stage_mesh_collapse_costs(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const double *quadrics,
                                             const rsm_mesh_decimate_params *p, uint64_t *keys, int32_t *multiplicity, double *cost, int32_t *reject, float *position,
                                             int64_t *n_edges) {
    if (!c) return RSM_E_INVALID;
    int s = meshdecimate_params_ok(c, p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_decimate", nv, nf)) != RSM_OK) return s;
    if (!n_edges || (nv > 0 && (!xyz || !quadrics)) || (nf > 0 && (!faces || !keys || !multiplicity || !cost || !reject || !position)))
        return set_err(c, RSM_E_INVALID, "mesh_decimate: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = 3 * (size_t)nf;
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv);
    int32_t *df = T.up(faces, n);
    double *dq = T.up(quadrics, 10 * (size_t)nv);
    uint64_t *dk = T.alloc<uint64_t>(n);
    int32_t *dm = T.alloc<int32_t>(n), *dr = T.alloc<int32_t>(n);
    double *dc = T.alloc<double>(n);
    float *dp = T.alloc<float>(3 * n);
    if (!dv || !df || !dq || !dk || !dm || !dr || !dc || !dp) return set_err(c, RSM_E_NOMEM, "mesh_decimate: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_collapse_costs_device(dv, nv, df, nf, dq, p, dk, dm, dc, dr, dp, n_edges, &invalid, c->stream)) != RSM_OK) return mesh_fail(c, "mesh_decimate", s, invalid);
    const size_t ne = (size_t)*n_edges;
    T.later(keys, dk, ne).later(multiplicity, dm, ne).later(cost, dc, ne).later(reject, dr, ne).later(position, dp, 3 * ne);
    return finish(c, T);
}

extern "C" int rsm_stage_mesh_collapse_round(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const double *quadrics,
                                             const rsm_mesh_decimate_params *p, int64_t need, float *out_xyz, int32_t *out_faces, double *out_quadrics,
                                             int64_t *n_faces_out, uint64_t *selected_keys, int64_t *n_selected, int64_t *n_kept) {
    if (!c) return RSM_E_INVALID;
    int s = meshdecimate_params_ok(c, p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_decimate", nv, nf)) != RSM_OK) return s;
    if (need < 0) return set_err(c, RSM_E_INVALID, "mesh_decimate: need %lld < 0", (long long)need);
    if (!n_faces_out || !n_selected || !n_kept || (nv > 0 && (!xyz || !quadrics || !out_xyz || !out_quadrics)) || (nf > 0 && (!faces || !out_faces || !selected_keys)))
        return set_err(c, RSM_E_INVALID, "mesh_decimate: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = 3 * (size_t)nf;
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv);
    int32_t *df = T.up(faces, n), *dfo = T.alloc<int32_t>(n);
    double *dq = T.up(quadrics, 10 * (size_t)nv);
    uint64_t *ds = T.alloc<uint64_t>(n);
    if (!dv || !df || !dfo || !dq || !ds) return set_err(c, RSM_E_NOMEM, "mesh_decimate: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_collapse_round_device(dv, nv, df, nf, dq, p, need, dfo, n_faces_out, ds, n_selected, n_kept, &invalid, c->stream)) != RSM_OK)
        return mesh_fail(c, "mesh_decimate", s, invalid);
    T.later(out_xyz, dv, 3 * (size_t)nv).later(out_quadrics, dq, 10 * (size_t)nv);
    T.later(out_faces, dfo, 3 * (size_t)*n_faces_out).later(selected_keys, ds, (size_t)*n_selected);
    return finish(c, T);
}

// ---- the Loop subdivision of the final mesh (k_meshsubdivide.hip) ----------------------------------------------------------
static int meshsubdivide_params_ok(rsm_ctx *c, const rsm_mesh_subdivide_params *p) {
    if (!p) return set_err(c, RSM_E_INVALID, "mesh_subdivide: params is NULL");
    if (p->iterations < 1 || p->iterations > 8) return set_err(c, RSM_E_INVALID, "mesh_subdivide: iterations %d outside 1..8", p->iterations);
    if (!std::isfinite(p->threshold) || p->threshold < 0.0) return set_err(c, RSM_E_INVALID, "mesh_subdivide: threshold %g negative or not finite", p->threshold);
    if (!(p->threshold_fraction >= 0.0 && p->threshold_fraction <= 1.0))
        return set_err(c, RSM_E_INVALID, "mesh_subdivide: threshold_fraction %g outside [0, 1]", p->threshold_fraction);
    if (p->weight_scheme != 0)
        return set_err(c, RSM_E_INVALID, "mesh_subdivide: weight_scheme %d not 0 (only Loop's own weights are built: LoopWeight 1 and 2 rest on tables this library does not have)",
                       p->weight_scheme);
    return RSM_OK;
}
extern "C" int rsm_mesh_subdivide_device(rsm_ctx *c, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_mesh_subdivide_params *p,
                                         int64_t *n_vertices, int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_subdivide", MeshIn{MESH_DEVICE, d_xyz, nv, d_faces, nf}, p, meshsubdivide_params_ok, mesh_subdivide_device, n_vertices, n_faces, stats);
}
extern "C" int rsm_mesh_subdivide(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_subdivide_params *p, int64_t *n_vertices,
                                  int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_subdivide", MeshIn{MESH_HOST, xyz, nv, faces, nf}, p, meshsubdivide_params_ok, mesh_subdivide_device, n_vertices, n_faces, stats);
}
extern "C" int rsm_mesh_subdivide_last(rsm_ctx *c, const rsm_mesh_subdivide_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats) {
    return mesh_stage_p(c, "mesh_subdivide", MeshIn{MESH_LAST}, p, meshsubdivide_params_ok, mesh_subdivide_device, n_vertices, n_faces, stats);
}

extern "C" int rsm_stage_mesh_subdivide_edges(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_subdivide_params *p,
                                              uint64_t *keys, int32_t *multiplicity, int32_t *split, float *odd_position, int64_t *n_edges, int32_t *vertex_class,
                                              float *even_position, double *thr) {
    if (!c) return RSM_E_INVALID;
    int s = meshsubdivide_params_ok(c, p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_subdivide", nv, nf)) != RSM_OK) return s;
    if (!n_edges || (nv > 0 && (!xyz || !vertex_class || !even_position)) || (nf > 0 && (!faces || !keys || !multiplicity || !split || !odd_position)))
        return set_err(c, RSM_E_INVALID, "mesh_subdivide: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = 3 * (size_t)nf;
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv), *dodd = T.alloc<float>(3 * n), *deven = T.alloc<float>(3 * (size_t)nv);
    int32_t *df = T.up(faces, n), *dm = T.alloc<int32_t>(n), *ds = T.alloc<int32_t>(n), *dc = T.alloc<int32_t>((size_t)nv);
    uint64_t *dk = T.alloc<uint64_t>(n);
    if (!dv || !df || !dodd || !deven || !dm || !ds || !dc || !dk) return set_err(c, RSM_E_NOMEM, "mesh_subdivide: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_subdivide_edges_device(dv, nv, df, nf, p, dk, dm, ds, dodd, n_edges, dc, deven, thr, &invalid, c->stream)) != RSM_OK)
        return mesh_fail(c, "mesh_subdivide", s, invalid);
    const size_t ne = (size_t)*n_edges;
    T.later(keys, dk, ne).later(multiplicity, dm, ne).later(split, ds, ne).later(odd_position, dodd, 3 * ne);
    T.later(vertex_class, dc, (size_t)nv).later(even_position, deven, 3 * (size_t)nv);
    return finish(c, T);
}

// ---- colours of the mesh from the rig's views (k_meshcolor.hip) ----------------------------------------------------------
static int meshcolor_params_ok(rsm_ctx *c, const rsm_mesh_color_params *p) {
    if (!p) return set_err(c, RSM_E_INVALID, "mesh_color: params is NULL");
    if (p->mode != 0 && p->mode != 1) return set_err(c, RSM_E_INVALID, "mesh_color: mode %d not 0 (best view) or 1 (blend)", p->mode);
    if (!(p->min_cos >= -1.0 && p->min_cos < 1.0)) return set_err(c, RSM_E_INVALID, "mesh_color: min_cos %g outside [-1, 1)", p->min_cos);
    if (!std::isfinite(p->depth_eps) || p->depth_eps < 0.0) return set_err(c, RSM_E_INVALID, "mesh_color: depth_eps %g negative or not finite", p->depth_eps);
    return RSM_OK;
}
static int meshcolor_views_ok(rsm_ctx *c, int64_t nv, const rsm_dedup_view *v, int np) {
    if (nv == 0) return RSM_OK;
    if (np < 1 || np > 32767) return set_err(c, RSM_E_INVALID, "mesh_color: n_pairs %d outside 1..32767", np);
    if (!v) return set_err(c, RSM_E_INVALID, "mesh_color: a NULL pointer (views)");
    for (int i = 0; i < np; i++) {
        if (v[i].width < 1 || v[i].height < 1) return set_err(c, RSM_E_INVALID, "mesh_color: pair %d: width %d / height %d < 1", i, v[i].width, v[i].height);
        if (!v[i].image[0] || !v[i].image[1]) return set_err(c, RSM_E_INVALID, "mesh_color: pair %d: a NULL pointer (image)", i);
    }
    return RSM_OK;
}
static int meshcolor_fail(rsm_ctx *c, int s, int invalid) {
    if (s == RSM_E_INVALID)
        return set_err(c, s, invalid == 1 ? "mesh_color: a face index outside [0, nv)" : invalid == 2 ? "mesh_color: a coordinate that is not finite"
                                                                                                       : "mesh_color: a singular P (det of its left 3x3 is 0)");
    return set_err(c, s, "mesh_color: failed%s", hip_tail(s).c_str());
}

extern "C" int rsm_mesh_color_device(rsm_ctx *c, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                                     const rsm_mesh_color_params *p, uint8_t *d_rgb, int32_t *d_best_view, double *stats) {
    if (!c) return RSM_E_INVALID;
    int s = meshcolor_params_ok(c, p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_color", nv, nf)) != RSM_OK) return s;
    if ((nv > 0 && (!d_xyz || !d_rgb)) || (nf > 0 && !d_faces)) return set_err(c, RSM_E_INVALID, "mesh_color: a NULL pointer");
    if ((s = meshcolor_views_ok(c, nv, views, n_pairs)) != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    int invalid = 0;
    s = mesh_color_device(d_xyz, nv, d_faces, nf, views, n_pairs, p, c->opt_meshcolor_big_box, d_rgb, d_best_view, stats, &invalid, c->stream);
    return s == RSM_OK ? RSM_OK : meshcolor_fail(c, s, invalid);
}

extern "C" int rsm_mesh_color(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                              const rsm_mesh_color_params *p, uint8_t *rgb, int32_t *best_view, double *stats) {
    if (!c) return RSM_E_INVALID;
    int s = meshcolor_params_ok(c, p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_color", nv, nf)) != RSM_OK) return s;
    if ((nv > 0 && (!xyz || !rgb)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_color: a NULL pointer");
    if ((s = meshcolor_views_ok(c, nv, views, n_pairs)) != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *db = T.alloc<int32_t>((size_t)nv);
    uint8_t *dc = T.alloc<uint8_t>(3 * (size_t)nv);
    if (!dv || !df || !db || !dc) return set_err(c, RSM_E_NOMEM, "mesh_color: no device memory for %lld vertices, %lld faces", (long long)nv, (long long)nf);
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    s = mesh_color_device(dv, nv, df, nf, views, n_pairs, p, c->opt_meshcolor_big_box, dc, db, stats, &invalid, c->stream);
    if (s != RSM_OK) return meshcolor_fail(c, s, invalid);
    T.later(rgb, dc, 3 * (size_t)nv).later(best_view, db, (size_t)nv);
    return finish(c, T);
}

// the context's colour buffers for a mesh of nv vertices (what rsm_mesh_last_colors copies out), without an owner yet
static int mcol_reserve(rsm_ctx *c, const char *who, int64_t nv) {
    if (c->mcol_rgb) (void)hipFree(c->mcol_rgb);
    if (c->mcol_best) (void)hipFree(c->mcol_best);
    c->mcol_rgb = nullptr;
    c->mcol_best = nullptr;
    c->mcol_valid = false;
    if (hipMalloc((void **)&c->mcol_rgb, 3 * (size_t)nv + 64) != hipSuccess || hipMalloc((void **)&c->mcol_best, sizeof(int32_t) * (size_t)nv + 64) != hipSuccess)
        return set_err(c, RSM_E_NOMEM, "%s: no device memory for %lld vertices", who, (long long)nv);
    return RSM_OK;
}

extern "C" int rsm_mesh_color_last(rsm_ctx *c, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *p, double *stats) {
    if (!c) return RSM_E_INVALID;
    int s = meshcolor_params_ok(c, p);
    const int64_t nv = c->pmesh.nv, nf = c->pmesh.nf;
    if (s != RSM_OK || (s = meshcolor_views_ok(c, nv, views, n_pairs)) != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = mcol_reserve(c, "mesh_color", nv)) != RSM_OK) return s;
    int invalid = 0;
    s = mesh_color_device(c->pmesh.d_v, nv, c->pmesh.d_f, nf, views, n_pairs, p, c->opt_meshcolor_big_box, c->mcol_rgb, c->mcol_best, stats, &invalid, c->stream);
    if (s != RSM_OK) return meshcolor_fail(c, s, invalid);
    c->mcol_valid = true;
    return RSM_OK;
}

extern "C" int rsm_mesh_last_colors(rsm_ctx *c, uint8_t *rgb, int32_t *best_view) {
    if (!c) return RSM_E_INVALID;
    if (!c->mcol_rgb || !c->mcol_valid)
        return set_err(c, RSM_E_STATE, "mesh_last_colors: the context's last mesh has no colours (rsm_mesh_color_last first)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nv = (size_t)c->pmesh.nv; // (valid: the mesh is the one they were computed on)
    if (rgb && nv > 0) HIPCHK(c, hipMemcpyAsync(rgb, c->mcol_rgb, 3 * nv, hipMemcpyDeviceToHost, c->stream));
    if (best_view && nv > 0) HIPCHK(c, hipMemcpyAsync(best_view, c->mcol_best, sizeof(int32_t) * nv, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RSM_OK;
}

extern "C" int rsm_texture_color(rsm_ctx *c, const float *xyz, int64_t n, const double P12[12], const uint8_t *image, int width, int height, uint8_t *rgb) {
    if (!c) return RSM_E_INVALID;
    if (n < 0 || n > (int64_t)INT32_MAX) return set_err(c, RSM_E_INVALID, "texture_color: n %lld outside 0..INT32_MAX", (long long)n);
    if (width < 1 || height < 1) return set_err(c, RSM_E_INVALID, "texture_color: width %d / height %d < 1", width, height);
    if (!P12 || !image || (n > 0 && (!xyz || !rgb))) return set_err(c, RSM_E_INVALID, "texture_color: a NULL pointer");
    if (n == 0) return RSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    const size_t pix = (size_t)width * (size_t)height;
    float *dp = T.up(xyz, 3 * (size_t)n);
    uint8_t *di = T.up(image, 3 * pix), *dc = T.alloc<uint8_t>(3 * (size_t)n);
    if (!dp || !di || !dc) return set_err(c, RSM_E_NOMEM, "texture_color: no device memory");
    const int s = texture_color_device(dp, n, P12, di, width, height, dc, c->stream);
    if (s != RSM_OK) return set_err(c, s, "texture_color: failed");
    HIPCHK(c, hipMemcpyAsync(rgb, dc, 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    return finish(c, T);
}

extern "C" int rsm_stage_mesh_depth(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const double P12[12], int width, int height,
                                    uint32_t *wbuf) {
    if (!c) return RSM_E_INVALID;
    int s = mesh_counts_ok(c, "mesh_color", nv, nf);
    if (s != RSM_OK) return s;
    if (width < 1 || height < 1) return set_err(c, RSM_E_INVALID, "mesh_color: width %d / height %d < 1", width, height);
    if (!P12 || !wbuf || (nv > 0 && !xyz) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_color: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    const size_t pix = (size_t)width * (size_t)height;
    float *dv = T.up(xyz, 3 * (size_t)nv);
    int32_t *df = T.up(faces, 3 * (size_t)nf);
    uint32_t *dw = T.alloc<uint32_t>(pix);
    if (!dv || !df || !dw) return set_err(c, RSM_E_NOMEM, "mesh_color: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_depth_device(dv, nv, df, nf, P12, width, height, c->opt_meshcolor_big_box, dw, &invalid, c->stream)) != RSM_OK) return meshcolor_fail(c, s, invalid);
    T.later(wbuf, dw, pix);
    return finish(c, T);
}

// ---- the views' exposure seams levelled in those colours (k_meshstitch.hip) ---------------------------------------------
static int meshstitch_params_ok(rsm_ctx *c, const rsm_mesh_color_params *p, const rsm_mesh_stitch_params *sp, int64_t nv, int n_pairs) {
    int s = meshcolor_params_ok(c, p);
    if (s != RSM_OK) return s;
    if (p->mode != 0) return set_err(c, RSM_E_INVALID, "mesh_stitch: mode %d not 0 (the best view's colours are what it levels)", p->mode);
    if (!sp) return set_err(c, RSM_E_INVALID, "mesh_stitch: stitch params is NULL");
    if (!std::isfinite(sp->lambda) || !(sp->lambda > 0.0)) return set_err(c, RSM_E_INVALID, "mesh_stitch: lambda %g not finite or not > 0", sp->lambda);
    if (sp->iterations < 0 || sp->iterations > RSM_MESH_STITCH_MAX_ITERATIONS)
        return set_err(c, RSM_E_INVALID, "mesh_stitch: iterations %d outside 0..%d", sp->iterations, RSM_MESH_STITCH_MAX_ITERATIONS);
    if (sp->iterations == 0 && !(sp->reduction > 0.0 && sp->reduction < 1.0)) return set_err(c, RSM_E_INVALID, "mesh_stitch: reduction %g not in (0, 1)", sp->reduction);
    if (sp->seam_gradient != 0 && sp->seam_gradient != 1) return set_err(c, RSM_E_INVALID, "mesh_stitch: seam_gradient %d not 0 or 1", sp->seam_gradient);
    if (nv > 0 && n_pairs > 32) return set_err(c, RSM_E_INVALID, "mesh_stitch: V = 2 n_pairs = %d views, more than the 64 a visibility mask holds", 2 * n_pairs);
    return RSM_OK;
}
static int meshstitch_fail(rsm_ctx *c, int s, int invalid) {
    if (s == RSM_E_INVALID && invalid == 4)
        return set_err(c, s, "mesh_stitch: reduction needs more than %d steps at this lambda (give iterations)", RSM_MESH_STITCH_MAX_ITERATIONS);
    return meshcolor_fail(c, s, invalid);
}

extern "C" int rsm_mesh_stitch_device(rsm_ctx *c, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                                      const rsm_mesh_color_params *p, const rsm_mesh_stitch_params *sp, uint8_t *d_rgb, int32_t *d_best_view, double *stats) {
    if (!c) return RSM_E_INVALID;
    int s = meshstitch_params_ok(c, p, sp, nv, n_pairs);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_color", nv, nf)) != RSM_OK) return s;
    if ((nv > 0 && (!d_xyz || !d_rgb)) || (nf > 0 && !d_faces)) return set_err(c, RSM_E_INVALID, "mesh_color: a NULL pointer");
    if ((s = meshcolor_views_ok(c, nv, views, n_pairs)) != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    int invalid = 0;
    s = mesh_stitch_device(d_xyz, nv, d_faces, nf, views, n_pairs, p, sp, c->opt_meshcolor_big_box, d_rgb, d_best_view, stats, &invalid, c->stream);
    return s == RSM_OK ? RSM_OK : meshstitch_fail(c, s, invalid);
}

extern "C" int rsm_mesh_stitch(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                               const rsm_mesh_color_params *p, const rsm_mesh_stitch_params *sp, uint8_t *rgb, int32_t *best_view, double *stats) {
    if (!c) return RSM_E_INVALID;
    int s = meshstitch_params_ok(c, p, sp, nv, n_pairs);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_color", nv, nf)) != RSM_OK) return s;
    if ((nv > 0 && (!xyz || !rgb)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_color: a NULL pointer");
    if ((s = meshcolor_views_ok(c, nv, views, n_pairs)) != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *db = T.alloc<int32_t>((size_t)nv);
    uint8_t *dc = T.alloc<uint8_t>(3 * (size_t)nv);
    if (!dv || !df || !db || !dc) return set_err(c, RSM_E_NOMEM, "mesh_stitch: no device memory for %lld vertices, %lld faces", (long long)nv, (long long)nf);
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    s = mesh_stitch_device(dv, nv, df, nf, views, n_pairs, p, sp, c->opt_meshcolor_big_box, dc, db, stats, &invalid, c->stream);
    if (s != RSM_OK) return meshstitch_fail(c, s, invalid);
    T.later(rgb, dc, 3 * (size_t)nv).later(best_view, db, (size_t)nv);
    return finish(c, T);
}

extern "C" int rsm_mesh_stitch_last(rsm_ctx *c, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *p, const rsm_mesh_stitch_params *sp,
                                    double *stats) {
    if (!c) return RSM_E_INVALID;
    const int64_t nv = c->pmesh.nv, nf = c->pmesh.nf;
    int s = meshstitch_params_ok(c, p, sp, nv, n_pairs);
    if (s != RSM_OK || (s = meshcolor_views_ok(c, nv, views, n_pairs)) != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = mcol_reserve(c, "mesh_stitch", nv)) != RSM_OK) return s;
    int invalid = 0;
    s = mesh_stitch_device(c->pmesh.d_v, nv, c->pmesh.d_f, nf, views, n_pairs, p, sp, c->opt_meshcolor_big_box, c->mcol_rgb, c->mcol_best, stats, &invalid, c->stream);
    if (s != RSM_OK) return meshstitch_fail(c, s, invalid);
    c->mcol_valid = true;
    return RSM_OK;
}

extern "C" int rsm_stage_mesh_visibility(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                                         const rsm_mesh_color_params *p, uint64_t *vis) {
    if (!c) return RSM_E_INVALID;
    int s = meshcolor_params_ok(c, p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_color", nv, nf)) != RSM_OK) return s;
    if ((nv > 0 && (!xyz || !vis)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_color: a NULL pointer");
    if ((s = meshcolor_views_ok(c, nv, views, n_pairs)) != RSM_OK) return s;
    if (nv > 0 && n_pairs > 32) return set_err(c, RSM_E_INVALID, "mesh_stitch: V = 2 n_pairs = %d views, more than the 64 a visibility mask holds", 2 * n_pairs);
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv);
    int32_t *df = T.up(faces, 3 * (size_t)nf);
    unsigned long long *dm = T.alloc<unsigned long long>((size_t)nv);
    if (!dv || !df || !dm) return set_err(c, RSM_E_NOMEM, "mesh_stitch: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_visibility_device(dv, nv, df, nf, views, n_pairs, p, c->opt_meshcolor_big_box, dm, &invalid, c->stream)) != RSM_OK) return meshcolor_fail(c, s, invalid);
    T.later(vis, (const uint64_t *)dm, (size_t)nv);
    return finish(c, T);
}

extern "C" int rsm_stage_mesh_stitch_rhs(rsm_ctx *c, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                                         const uint8_t *rgb, const int32_t *best_view, const uint64_t *vis, int seam_gradient, double *G, int32_t *deg,
                                         int64_t counts[5]) {
    if (!c) return RSM_E_INVALID;
    int s = mesh_counts_ok(c, "mesh_color", nv, nf);
    if (s != RSM_OK) return s;
    if (!counts || (nv > 0 && (!xyz || !rgb || !best_view || !vis || !G || !deg)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_stitch: a NULL pointer");
    if (seam_gradient != 0 && seam_gradient != 1) return set_err(c, RSM_E_INVALID, "mesh_stitch: seam_gradient %d not 0 or 1", seam_gradient);
    if ((s = meshcolor_views_ok(c, nv, views, n_pairs)) != RSM_OK) return s;
    if (nv > 0 && n_pairs > 32) return set_err(c, RSM_E_INVALID, "mesh_stitch: V = 2 n_pairs = %d views, more than the 64 a visibility mask holds", 2 * n_pairs);
    for (int64_t i = 0; i < nv; i++)
        if (best_view[i] < -1 || best_view[i] >= 2 * n_pairs) return set_err(c, RSM_E_INVALID, "mesh_stitch: best_view[%lld] = %d outside -1..V-1", (long long)i, best_view[i]);
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    float *dv = T.up(xyz, 3 * (size_t)nv);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *db = T.up(best_view, (size_t)nv), *dd = T.alloc<int32_t>((size_t)nv);
    uint8_t *dc = T.up(rgb, 3 * (size_t)nv);
    unsigned long long *dm = T.up((const unsigned long long *)vis, (size_t)nv);
    double *dG = T.alloc<double>(3 * (size_t)nv);
    if (!dv || !df || !db || !dd || !dc || !dm || !dG) return set_err(c, RSM_E_NOMEM, "mesh_stitch: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_stitch_rhs_device(dv, nv, df, nf, views, n_pairs, dc, db, dm, seam_gradient, dG, dd, counts, &invalid, c->stream)) != RSM_OK)
        return meshcolor_fail(c, s, invalid);
    T.later(G, dG, 3 * (size_t)nv).later(deg, dd, (size_t)nv);
    return finish(c, T);
}

extern "C" int rsm_stage_mesh_stitch_solve(rsm_ctx *c, const int32_t *faces, int64_t nv, int64_t nf, const int32_t *best_view, const uint8_t *rgb, const double *G,
                                           double lambda, int iterations, double *x, double *rel_residual) {
    if (!c) return RSM_E_INVALID;
    int s = mesh_counts_ok(c, "mesh_color", nv, nf);
    if (s != RSM_OK) return s;
    if (!rel_residual || (nv > 0 && (!best_view || !rgb || !G || !x)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_stitch: a NULL pointer");
    if (!std::isfinite(lambda) || !(lambda > 0.0)) return set_err(c, RSM_E_INVALID, "mesh_stitch: lambda %g not finite or not > 0", lambda);
    if (iterations < 0 || iterations > RSM_MESH_STITCH_MAX_ITERATIONS)
        return set_err(c, RSM_E_INVALID, "mesh_stitch: iterations %d outside 0..%d", iterations, RSM_MESH_STITCH_MAX_ITERATIONS);
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *db = T.up(best_view, (size_t)nv);
    uint8_t *dc = T.up(rgb, 3 * (size_t)nv);
    double *dG = T.up(G, 3 * (size_t)nv), *dx = T.alloc<double>(3 * (size_t)nv);
    if (!df || !db || !dc || !dG || !dx) return set_err(c, RSM_E_NOMEM, "mesh_stitch: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_stitch_solve_device(df, nv, nf, db, dc, dG, lambda, iterations, dx, rel_residual, &invalid, c->stream)) != RSM_OK) return meshcolor_fail(c, s, invalid);
    T.later(x, dx, 3 * (size_t)nv);
    return finish(c, T);
}

// ---- the vertices no view sees filled from the colours around them (k_meshfill.hip) -------------------------------------
static int meshfill_params_ok(rsm_ctx *c, const rsm_mesh_fill_params *p) {
    if (!p) return set_err(c, RSM_E_INVALID, "mesh_fill: params is NULL");
    if (p->max_rounds < 0) return set_err(c, RSM_E_INVALID, "mesh_fill: max_rounds %d < 0", p->max_rounds);
    if (p->iterations < 0 || p->iterations > RSM_MESH_FILL_MAX_ITERATIONS)
        return set_err(c, RSM_E_INVALID, "mesh_fill: iterations %d outside 0..%d", p->iterations, RSM_MESH_FILL_MAX_ITERATIONS);
    if (p->iterations == 0 && !(p->reduction > 0.0 && p->reduction < 1.0)) return set_err(c, RSM_E_INVALID, "mesh_fill: reduction %g not in (0, 1)", p->reduction);
    return RSM_OK;
}
static int meshfill_fail(rsm_ctx *c, int s, int invalid) {
    if (s == RSM_E_INVALID && invalid == 4)
        return set_err(c, s, "mesh_fill: reduction needs more than %d steps on a front this deep (give iterations)", RSM_MESH_FILL_MAX_ITERATIONS);
    if (s == RSM_E_INVALID) return set_err(c, s, "mesh_fill: a face index outside [0, nv)");
    return set_err(c, s, "mesh_fill: failed%s", hip_tail(s).c_str());
}

extern "C" int rsm_mesh_fill_colors_device(rsm_ctx *c, const int32_t *d_faces, int64_t nv, int64_t nf, uint8_t *d_rgb, const int32_t *d_best_view, int32_t *d_level,
                                           const rsm_mesh_fill_params *p, double *stats) {
    if (!c) return RSM_E_INVALID;
    int s = meshfill_params_ok(c, p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_fill", nv, nf)) != RSM_OK) return s;
    if ((nv > 0 && (!d_rgb || !d_best_view)) || (nf > 0 && !d_faces)) return set_err(c, RSM_E_INVALID, "mesh_fill: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    int invalid = 0;
    s = mesh_fill_device(d_faces, nv, nf, d_best_view, d_rgb, d_level, p, RSM_MESH_FILL_ROUND_BATCH, stats, &invalid, c->stream);
    return s == RSM_OK ? RSM_OK : meshfill_fail(c, s, invalid);
}

extern "C" int rsm_mesh_fill_colors(rsm_ctx *c, const int32_t *faces, int64_t nv, int64_t nf, uint8_t *rgb, const int32_t *best_view, int32_t *level,
                                    const rsm_mesh_fill_params *p, double *stats) {
    if (!c) return RSM_E_INVALID;
    int s = meshfill_params_ok(c, p);
    if (s != RSM_OK || (s = mesh_counts_ok(c, "mesh_fill", nv, nf)) != RSM_OK) return s;
    if ((nv > 0 && (!rgb || !best_view)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_fill: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *db = T.up(best_view, (size_t)nv), *dl = T.alloc<int32_t>((size_t)nv);
    uint8_t *dc = T.up((const uint8_t *)rgb, 3 * (size_t)nv);
    if (!df || !db || !dl || !dc) return set_err(c, RSM_E_NOMEM, "mesh_fill: no device memory for %lld vertices, %lld faces", (long long)nv, (long long)nf);
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    s = mesh_fill_device(df, nv, nf, db, dc, dl, p, RSM_MESH_FILL_ROUND_BATCH, stats, &invalid, c->stream);
    if (s != RSM_OK) return meshfill_fail(c, s, invalid);
    T.later(rgb, (const uint8_t *)dc, 3 * (size_t)nv).later(level, (const int32_t *)dl, (size_t)nv);
    return finish(c, T);
}

extern "C" int rsm_mesh_fill_colors_last(rsm_ctx *c, const rsm_mesh_fill_params *p, double *stats) {
    if (!c) return RSM_E_INVALID;
    int s = meshfill_params_ok(c, p);
    if (s != RSM_OK) return s;
    if (!c->mcol_rgb || !c->mcol_best || !c->mcol_valid)
        return set_err(c, RSM_E_STATE, "mesh_fill: the context's last mesh has no colours (rsm_mesh_color_last or rsm_mesh_stitch_last first)");
    HIPCHK(c, hipSetDevice(c->device));
    int invalid = 0;
    s = mesh_fill_device(c->pmesh.d_f, c->pmesh.nv, c->pmesh.nf, c->mcol_best, c->mcol_rgb, nullptr, p, RSM_MESH_FILL_ROUND_BATCH, stats, &invalid, c->stream);
    return s == RSM_OK ? RSM_OK : meshfill_fail(c, s, invalid);
}

extern "C" int rsm_stage_mesh_fill_front(rsm_ctx *c, const int32_t *faces, int64_t nv, int64_t nf, const uint8_t *rgb, const int32_t *best_view, int max_rounds,
                                         int round_batch, double *x, int32_t *level, int *rounds) {
    if (!c) return RSM_E_INVALID;
    int s = mesh_counts_ok(c, "mesh_fill", nv, nf);
    if (s != RSM_OK) return s;
    if (!rounds || (nv > 0 && (!rgb || !best_view || !x || !level)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_fill: a NULL pointer");
    if (max_rounds < 0) return set_err(c, RSM_E_INVALID, "mesh_fill: max_rounds %d < 0", max_rounds);
    if (round_batch < 0 || round_batch > 1024) return set_err(c, RSM_E_INVALID, "mesh_fill: round_batch %d outside 0..1024", round_batch);
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *db = T.up(best_view, (size_t)nv), *dl = T.alloc<int32_t>((size_t)nv);
    uint8_t *dc = T.up(rgb, 3 * (size_t)nv);
    double *dx = T.alloc<double>(3 * (size_t)nv);
    if (!df || !db || !dl || !dc || !dx) return set_err(c, RSM_E_NOMEM, "mesh_fill: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_fill_front_device(df, nv, nf, db, dc, max_rounds, round_batch ? round_batch : RSM_MESH_FILL_ROUND_BATCH, dx, dl, rounds, &invalid, c->stream)) != RSM_OK)
        return meshfill_fail(c, s, invalid);
    T.later(x, (const double *)dx, 3 * (size_t)nv).later(level, (const int32_t *)dl, (size_t)nv);
    return finish(c, T);
}

extern "C" int rsm_stage_mesh_fill_solve(rsm_ctx *c, const int32_t *faces, int64_t nv, int64_t nf, const int32_t *level, int L, int iterations, double *x) {
    if (!c) return RSM_E_INVALID;
    int s = mesh_counts_ok(c, "mesh_fill", nv, nf);
    if (s != RSM_OK) return s;
    if ((nv > 0 && (!level || !x)) || (nf > 0 && !faces)) return set_err(c, RSM_E_INVALID, "mesh_fill: a NULL pointer");
    if (L < 0) return set_err(c, RSM_E_INVALID, "mesh_fill: L %d < 0", L);
    if (iterations < 0 || iterations > RSM_MESH_FILL_MAX_ITERATIONS)
        return set_err(c, RSM_E_INVALID, "mesh_fill: iterations %d outside 0..%d", iterations, RSM_MESH_FILL_MAX_ITERATIONS);
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c);
    int32_t *df = T.up(faces, 3 * (size_t)nf), *dl = T.up(level, (size_t)nv);
    double *dx = T.up((const double *)x, 3 * (size_t)nv);
    if (!df || !dl || !dx) return set_err(c, RSM_E_NOMEM, "mesh_fill: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int invalid = 0;
    if ((s = mesh_fill_solve_device(df, nv, nf, dl, L, iterations, dx, &invalid, c->stream)) != RSM_OK) return meshfill_fail(c, s, invalid);
    T.later(x, (const double *)dx, 3 * (size_t)nv);
    return finish(c, T);
}
