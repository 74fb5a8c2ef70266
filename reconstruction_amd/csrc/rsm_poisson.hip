// rsm_poisson.hip -- the host side of the Poisson surface: the checks of the four calls
// rsm_poisson_mesh{,_weighted,_banded,_banded_weighted}{,_device}, the one run behind them, and the stage entries of the tests.  A call is dense
// or banded (bp) and splats plainly or by density (dp); what the device side shares is in poisson_space.h.
#include "rsm_ctx.h"

#include <cmath>
#include <string.h>

// ---- the checks -----------------------------------------------------------------------------------------------------------------------------
static int poisson_params_ok(rsm_ctx *c, const rsm_poisson_params *p) {
    if (!p) return set_err(c, RSM_E_INVALID, "poisson: params is NULL");
    if (p->depth < 5 || p->depth > 9) return set_err(c, RSM_E_INVALID, "poisson: depth %d outside 5..9", p->depth);
    if (!std::isfinite(p->scale) || p->scale < 1.0) return set_err(c, RSM_E_INVALID, "poisson: scale %g not finite or < 1", p->scale);
    if (!(p->rel_residual > 0.0 && p->rel_residual < 1.0)) return set_err(c, RSM_E_INVALID, "poisson: rel_residual %g not in (0, 1)", p->rel_residual);
    if (p->max_cycles < 1) return set_err(c, RSM_E_INVALID, "poisson: max_cycles %d < 1", p->max_cycles);
    if (p->trim_cells < 0) return set_err(c, RSM_E_INVALID, "poisson: trim_cells %d < 0", p->trim_cells);
    return RSM_OK;
}
static int poisson_n_ok(rsm_ctx *c, int64_t n) {
    if (n < 0 || n > (int64_t)INT32_MAX) return set_err(c, RSM_E_INVALID, "poisson: n %lld outside 0..INT32_MAX", (long long)n);
    return RSM_OK;
}
static int poisson_fail(rsm_ctx *c, int s, const char *what) { return set_err(c, s, "poisson: %s failed%s", what, hip_tail(s).c_str()); }
static int poisson_density_params_ok(rsm_ctx *c, const rsm_poisson_params *p, const rsm_poisson_density_params *dp) {
    if (!dp) return set_err(c, RSM_E_INVALID, "poisson: density params is NULL");
    if (dp->kernel_depth != 0 && (dp->kernel_depth < 3 || dp->kernel_depth > p->depth))
        return set_err(c, RSM_E_INVALID, "poisson: kernel_depth %d neither 0 nor in 3..%d", dp->kernel_depth, p->depth);
    if (!std::isfinite(dp->samples_per_node) || !(dp->samples_per_node > 0.0))
        return set_err(c, RSM_E_INVALID, "poisson: samples_per_node %g not finite or <= 0", dp->samples_per_node);
    return RSM_OK;
}
static int poisson_depth_in_ok(rsm_ctx *c, const double *depth_in, int64_t n) {
    if (depth_in)
        for (int64_t i = 0; i < n; i++)
            if (!std::isfinite(depth_in[i])) return set_err(c, RSM_E_INVALID, "poisson: depth_in[%lld] is not finite", (long long)i);
    return RSM_OK;
}
static int density_kernel_depth(const rsm_poisson_params *p, const rsm_poisson_density_params *dp) { return dp->kernel_depth ? dp->kernel_depth : p->depth - 2; }
// p with its depth as the finest one; `coarse`: p as the dense solve at depth - 1 reads it
static int poisson_band_params_ok(rsm_ctx *c, const rsm_poisson_params *p, const rsm_poisson_band_params *bp, rsm_poisson_params *coarse) {
    if (!p) return set_err(c, RSM_E_INVALID, "poisson: params is NULL");
    if (!bp) return set_err(c, RSM_E_INVALID, "poisson: band params is NULL");
    if (p->depth < 6 || p->depth > 10) return set_err(c, RSM_E_INVALID, "poisson: banded depth %d outside 6..10", p->depth);
    *coarse = *p;
    coarse->depth = p->depth - 1;
    const int s = poisson_params_ok(c, coarse);
    if (s != RSM_OK) return s;
    if (bp->band_bricks < 1 || bp->band_bricks > 4) return set_err(c, RSM_E_INVALID, "poisson: band_bricks %d outside 1..4", bp->band_bricks);
    if (bp->max_iterations < 1) return set_err(c, RSM_E_INVALID, "poisson: max_iterations %d < 1", bp->max_iterations);
    if (p->trim_cells > 8 * bp->band_bricks - 1)
        return set_err(c, RSM_E_INVALID, "poisson: trim_cells %d > 8 band_bricks - 1 = %d (a kept face needs its cell in the band)", p->trim_cells, 8 * bp->band_bricks - 1);
    return RSM_OK;
}
static int poisson_band_cap(rsm_ctx *c, const PoissonBand &band, int64_t max_bricks) {
    if (band.n_active > max_bricks)
        return set_err(c, RSM_E_INVALID, "poisson: %lld active bricks, more than the %lld allowed (such a cloud fills the volume)", (long long)band.n_active,
                       (long long)max_bricks);
    return RSM_OK;
}
struct BandOwner { // frees a call's band on every way out
    PoissonBand b;
    ~BandOwner() { poisson_band_free(&b); }
};
// a caller's brick list: ascending, each in [0, B^3)
static int poisson_band_list_ok(rsm_ctx *c, const int32_t *bricks, int64_t n_bricks, int depth) {
    if (depth < 6 || depth > 10) return set_err(c, RSM_E_INVALID, "poisson: banded depth %d outside 6..10", depth);
    const int64_t B3 = (int64_t)1 << (3 * (depth - 3));
    if (n_bricks < 0 || n_bricks > B3 || n_bricks > RSM_POISSON_BAND_MAX_BRICKS)
        return set_err(c, RSM_E_INVALID, "poisson: n_bricks %lld outside 0..min(B^3, 2^20)", (long long)n_bricks);
    if (n_bricks > 0 && !bricks) return set_err(c, RSM_E_INVALID, "poisson: a NULL pointer");
    for (int64_t i = 0; i < n_bricks; i++)
        if (bricks[i] < 0 || bricks[i] >= B3 || (i > 0 && bricks[i] <= bricks[i - 1]))
            return set_err(c, RSM_E_INVALID, "poisson: bricks[%lld] = %d out of range or not ascending", (long long)i, bricks[i]);
    return RSM_OK;
}
// f16's checks, then f14's with the kernel depth inside the coarse problem too
static int poisson_band_density_params_ok(rsm_ctx *c, const rsm_poisson_params *p, const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp,
                                          rsm_poisson_params *coarse) {
    int s = poisson_band_params_ok(c, p, bp, coarse);
    if (s != RSM_OK) return s;
    if (!dp) return set_err(c, RSM_E_INVALID, "poisson: density params is NULL");
    if (dp->kernel_depth != 0 && (dp->kernel_depth < 3 || dp->kernel_depth > p->depth - 1))
        return set_err(c, RSM_E_INVALID, "poisson: kernel_depth %d neither 0 nor in 3..%d (the banded call's density grid exists at depth - 1 too)", dp->kernel_depth,
                       p->depth - 1);
    return poisson_density_params_ok(c, p, dp);
}
// which of the four calls an entry is
struct PoissonCall {
    bool band, density;
};
// a call's checks before its pointers: the params in the call's order (`coarse`: a banded call's p as the dense solve at depth - 1 reads it), then n
static int poisson_call_ok(rsm_ctx *c, PoissonCall k, const rsm_poisson_params *p, const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp, int64_t n,
                           rsm_poisson_params *coarse) {
    int s = !k.band ? poisson_params_ok(c, p) : k.density ? poisson_band_density_params_ok(c, p, bp, dp, coarse) : poisson_band_params_ok(c, p, bp, coarse);
    if (s == RSM_OK && !k.band && k.density) s = poisson_density_params_ok(c, p, dp);
    return s != RSM_OK ? s : poisson_n_ok(c, n);
}

// ---- the run ------------------------------------------------------------------------------------------------------------------------------
// what a density call holds on the device per sample, and a banded one besides its band fields: the dense levels 3..depth - 1
struct DensityBufs {
    double *rho = nullptr, *w = nullptr, *d = nullptr;
    unsigned long long *levels = nullptr;
    bool alloc(Tmp &T, int64_t n, int depth, bool band) {
        rho = T.alloc<double>((size_t)n), w = T.alloc<double>((size_t)n), d = T.alloc<double>((size_t)n);
        if (band) levels = T.alloc<unsigned long long>(poisson_density_level_words(depth - 1));
        return rho && w && d && (levels || !band);
    }
};
// the coarse field of a banded call: f7's steps 3 to 5 at depth - 1 on the box of `grid` (the fine grid) -> chi_c; with D, f14's items 4 to 6 with the
// fine problem's w and d (clamped to depth - 1 where they are read) in place of f7's splat.  RSM_OK / RSM_W_NOT_CONVERGED / an error set
static int poisson_band_coarse(rsm_ctx *c, const float *d_xyz, const float *d_nrm, int64_t n, const rsm_poisson_params *coarse, const double grid[4],
                               const DensityBufs *D, float *chi_c, double *res, int *cycles) {
    const size_t C3 = (size_t)1 << (3 * coarse->depth);
    const double cgrid[4] = {grid[0], grid[1], grid[2], 2.0 * grid[3]};
    Tmp T(c);
    float *b = T.alloc<float>(C3);
    uint8_t *occ = D ? nullptr : T.alloc<uint8_t>(C3);
    if (!b || (!D && !occ)) return set_err(c, RSM_E_NOMEM, "poisson: no device memory for depth %d", coarse->depth);
    int s;
    if (D) {
        const double *U = nullptr;
        s = poisson_density_levels_device(d_xyz, d_nrm, n, coarse->depth, coarse->depth, cgrid, D->w, D->d, D->levels, nullptr, &U, c->stream);
        if (s == RSM_OK) poisson_density_rhs_of_field(U, coarse->depth, b, nullptr, c->stream);
    } else
        s = poisson_rhs_device(d_xyz, d_nrm, n, coarse->depth, cgrid, b, nullptr, occ, c->stream);
    if (s != RSM_OK) return poisson_fail(c, s, "coarse right-hand side");
    s = poisson_solve_device(b, coarse->depth, coarse->rel_residual, coarse->max_cycles, chi_c, res, cycles, nullptr, c->stream);
    return s < 0 ? poisson_fail(c, s, "coarse solve") : s;
}

// where the blocks of a call's stats sit (include/rsm.h): [0..11] are every call's; -1: the call has no such block
struct PoissonStatsLayout {
    int n;               // the call's stats
    int band_at;         // active bricks, occupied bricks, the coarse solve's cycles, its residual, the band residual before the solve
    int kernel_depth_at; // the kernel depth used
    int samples_at;      // the least d, the samples below the depth, the sum of w
};
static const PoissonStatsLayout poisson_stats_layout[2][2] = {
    // [banded][by density]
    {{RSM_POISSON_STATS, -1, -1, -1}, {RSM_POISSON_WEIGHTED_STATS, -1, 12, 13}},
    {{RSM_POISSON_BAND_STATS, 12, -1, -1}, {RSM_POISSON_BAND_WEIGHTED_STATS, 12, 17, 18}},
};

// A call on device buffers; the mesh lands in c->pmesh.  bp NULL: the dense grid; dp NULL: the plain splat; coarse: a banded call's coarse params
static int poisson_run(rsm_ctx *c, const float *d_xyz, const float *d_nrm, int64_t n, const rsm_poisson_params *p, const rsm_poisson_band_params *bp,
                       const rsm_poisson_density_params *dp, const rsm_poisson_params *coarse, int64_t *n_vertices, int64_t *n_faces, double *stats) {
    const PoissonStatsLayout at = poisson_stats_layout[bp != nullptr][dp != nullptr];
    double st[RSM_POISSON_BAND_WEIGHTED_STATS] = {0}, sample_stats[3] = {0.0, 0.0, 0.0};
    hipStream_t stream = c->stream;
    *n_vertices = *n_faces = 0;
    poisson_mesh_free(&c->pmesh);
    mesh_replaced(c);
    // grid
    double grid[4];
    int64_t counts[2];
    int s = poisson_grid_device(d_xyz, d_nrm, n, p->depth, p->scale, grid, counts, stream);
    if (s != RSM_OK) return poisson_fail(c, s, "bounding box");
    st[0] = (double)counts[0];
    st[1] = (double)counts[1];
    st[9] = (double)(1 << p->depth);
    const int kernel_depth = dp ? density_kernel_depth(p, dp) : 0;
    if (dp) st[at.kernel_depth_at] = (double)kernel_depth;
    int status = RSM_OK;
    if (grid[3] > 0.0) {
        // band
        BandOwner band;
        if (bp) {
            if ((s = poisson_band_bricks_device(d_xyz, d_nrm, n, p->depth, grid, bp->band_bricks, RSM_POISSON_BAND_MAX_BRICKS, &band.b, stream)) != RSM_OK)
                return poisson_fail(c, s, "bricks");
            if ((s = poisson_band_cap(c, band.b, RSM_POISSON_BAND_MAX_BRICKS)) != RSM_OK) return s;
        }
        // the call's fields: on the grid's nodes or the band's
        const size_t nodes = bp ? (size_t)band.b.n_active * 512 : (size_t)1 << (3 * p->depth);
        Tmp T(c);
        float *chi_c = bp ? T.alloc<float>((size_t)1 << (3 * coarse->depth)) : nullptr, *b = T.alloc<float>(nodes), *chi = T.alloc<float>(nodes);
        uint8_t *occ = T.alloc<uint8_t>(nodes);
        DensityBufs D;
        if ((dp && !D.alloc(T, n, p->depth, bp != nullptr)) || (bp && !chi_c) || !b || !chi || !occ)
            return bp ? set_err(c, RSM_E_NOMEM, "poisson: no device memory for %lld bricks at depth %d", (long long)band.b.n_active, p->depth)
                      : set_err(c, RSM_E_NOMEM, "poisson: no device memory for depth %d", p->depth);
        // the two steps that all four calls spell differently, and the word a failure of the first is reported under
        auto right_hand_side = [&](const char **what) -> int {
            *what = bp ? "band right-hand side" : dp ? "density-adaptive right-hand side" : "right-hand side";
            if (bp && dp) return poisson_band_density_rhs_device(band.b, d_xyz, d_nrm, n, grid, D.w, D.d, D.levels, b, nullptr, occ, stream);
            if (bp) return poisson_band_rhs_device(band.b, d_xyz, d_nrm, n, grid, b, nullptr, occ, stream);
            if (dp) // (takes the sample densities itself)
                return poisson_density_rhs_device(d_xyz, d_nrm, n, p->depth, grid, kernel_depth, dp->samples_per_node, nullptr, b, nullptr, occ, D.rho, D.w, D.d,
                                                  sample_stats, stream);
            return poisson_rhs_device(d_xyz, d_nrm, n, p->depth, grid, b, nullptr, occ, stream);
        };
        auto iso_value = [&](double *iso) -> int {
            if (bp && dp) return poisson_band_iso_weighted_device(band.b, d_xyz, d_nrm, n, D.w, sample_stats[2], chi, grid, iso, stream);
            if (bp) return poisson_band_iso_device(band.b, d_xyz, d_nrm, n, counts[0], chi, grid, iso, stream);
            if (dp) return poisson_iso_weighted_device(d_xyz, d_nrm, n, D.w, sample_stats[2], chi, p->depth, grid, iso, stream);
            return poisson_iso_device(d_xyz, d_nrm, n, counts[0], chi, p->depth, grid, iso, stream);
        };
        // sample densities (a banded call's; the dense call takes them inside its right-hand side)
        if (bp && dp &&
            (s = poisson_density_samples_device(d_xyz, d_nrm, n, p->depth, grid, kernel_depth, dp->samples_per_node, nullptr, D.rho, D.w, D.d, sample_stats, stream)) !=
                RSM_OK)
            return poisson_fail(c, s, "sample densities");
        // coarse field
        double cres = 0.0, res0 = 0.0, res = 0.0, iso = 0.0;
        int ccycles = 0, its = 0, csolved = RSM_OK;
        if (bp && (csolved = poisson_band_coarse(c, d_xyz, d_nrm, n, coarse, grid, dp ? &D : nullptr, chi_c, &cres, &ccycles)) < 0) return csolved;
        // right-hand side
        const char *what = nullptr;
        if ((s = right_hand_side(&what)) != RSM_OK) return poisson_fail(c, s, what);
        // guess
        if (bp && (s = poisson_band_guess_device(band.b, chi_c, chi, stream)) != RSM_OK) return poisson_fail(c, s, "guess");
        // solve
        const int solved = bp ? poisson_band_solve_device(band.b, b, chi_c, p->rel_residual, bp->max_iterations, chi, &res0, &res, &its, nullptr, stream)
                              : poisson_solve_device(b, p->depth, p->rel_residual, p->max_cycles, chi, &res, &its, nullptr, stream);
        if (solved < 0) return poisson_fail(c, solved, bp ? "band solve" : "solve");
        // iso
        if ((s = iso_value(&iso)) != RSM_OK) return poisson_fail(c, s, "iso-value");
        // extraction
        int64_t un[2];
        s = bp ? poisson_band_extract_device(band.b, chi, iso, grid, occ, p->trim_cells, &c->pmesh, un, stream)
               : poisson_extract_device(chi, p->depth, iso, grid, occ, p->trim_cells, &c->pmesh, un, stream);
        if (s != RSM_OK) return poisson_fail(c, s, "extraction");
        mesh_replaced(c);
        // stats
        st[2] = res;
        st[3] = (double)its;
        st[4] = iso;
        for (int a = 0; a < 4; a++) st[5 + a] = grid[a];
        st[10] = (double)un[0];
        st[11] = (double)un[1];
        if (at.band_at >= 0) {
            const double band_block[5] = {(double)band.b.n_active, (double)band.b.n_occupied, (double)ccycles, cres, res0};
            memcpy(&st[at.band_at], band_block, sizeof band_block);
        }
        if (at.samples_at >= 0) memcpy(&st[at.samples_at], sample_stats, sizeof sample_stats);
        if (solved == RSM_W_NOT_CONVERGED && bp) set_err(c, solved, "poisson: band residual %g after %d iterations (rel_residual %g)", res, its, p->rel_residual);
        else if (solved == RSM_W_NOT_CONVERGED) set_err(c, solved, "poisson: residual %g after %d cycles (rel_residual %g)", res, its, p->rel_residual);
        else if (csolved == RSM_W_NOT_CONVERGED) set_err(c, csolved, "poisson: coarse residual %g after %d cycles (rel_residual %g)", cres, ccycles, p->rel_residual);
        status = (solved == RSM_W_NOT_CONVERGED || csolved == RSM_W_NOT_CONVERGED) ? RSM_W_NOT_CONVERGED : RSM_OK;
    }
    *n_vertices = c->pmesh.nv;
    *n_faces = c->pmesh.nf;
    if (stats) memcpy(stats, st, sizeof(double) * (size_t)at.n);
    return status;
}

// ---- the eight entries: check, upload (the host entries), run --------------------------------------------------------------------------------
static int poisson_mesh_entry(rsm_ctx *c, PoissonCall k, bool on_device, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                              const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp, int64_t *n_vertices, int64_t *n_faces, double *stats) {
    if (!c) return RSM_E_INVALID;
    rsm_poisson_params coarse;
    int s = poisson_call_ok(c, k, p, bp, dp, n, &coarse);
    if (s != RSM_OK) return s;
    if (!n_vertices || !n_faces || (n > 0 && (!xyz || !normals4))) return set_err(c, RSM_E_INVALID, "poisson: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    Tmp T(c); // (the uploads of a host entry; they live until the run is over)
    if (!on_device) {
        float *dx = T.up(xyz, 3 * (size_t)n), *dn = T.up(normals4, 4 * (size_t)n);
        if (!dx || !dn) return set_err(c, RSM_E_NOMEM, "poisson: no device memory for %lld samples", (long long)n);
        if (n > 0 && (s = finish(c, T)) != RSM_OK) return s;
        xyz = dx, normals4 = dn;
    }
    return poisson_run(c, xyz, normals4, n, p, k.band ? bp : nullptr, k.density ? dp : nullptr, k.band ? &coarse : nullptr, n_vertices, n_faces, stats);
}
extern "C" int rsm_poisson_mesh(rsm_ctx *c, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p, int64_t *n_vertices,
    int64_t *n_faces, double *stats) {
    return poisson_mesh_entry(c, PoissonCall{false, false}, false, xyz, normals4, n, p, nullptr, nullptr, n_vertices, n_faces, stats);
}
extern "C" int rsm_poisson_mesh_device(rsm_ctx *c, const float *d_xyz, const float *d_normals4, int64_t n, const rsm_poisson_params *p, int64_t *n_vertices,
    int64_t *n_faces, double *stats) {
    return poisson_mesh_entry(c, PoissonCall{false, false}, true, d_xyz, d_normals4, n, p, nullptr, nullptr, n_vertices, n_faces, stats);
}
extern "C" int rsm_poisson_mesh_weighted(rsm_ctx *c, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p, const rsm_poisson_density_params *dp, int64_t *n_vertices,
    int64_t *n_faces, double *stats) {
    return poisson_mesh_entry(c, PoissonCall{false, true}, false, xyz, normals4, n, p, nullptr, dp, n_vertices, n_faces, stats);
}
extern "C" int rsm_poisson_mesh_weighted_device(rsm_ctx *c, const float *d_xyz, const float *d_normals4, int64_t n, const rsm_poisson_params *p, const rsm_poisson_density_params *dp, int64_t *n_vertices,
    int64_t *n_faces, double *stats) {
    return poisson_mesh_entry(c, PoissonCall{false, true}, true, d_xyz, d_normals4, n, p, nullptr, dp, n_vertices, n_faces, stats);
}
extern "C" int rsm_poisson_mesh_banded(rsm_ctx *c, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p, const rsm_poisson_band_params *bp, int64_t *n_vertices,
    int64_t *n_faces, double *stats) {
    return poisson_mesh_entry(c, PoissonCall{true, false}, false, xyz, normals4, n, p, bp, nullptr, n_vertices, n_faces, stats);
}
extern "C" int rsm_poisson_mesh_banded_device(rsm_ctx *c, const float *d_xyz, const float *d_normals4, int64_t n, const rsm_poisson_params *p, const rsm_poisson_band_params *bp, int64_t *n_vertices,
    int64_t *n_faces, double *stats) {
    return poisson_mesh_entry(c, PoissonCall{true, false}, true, d_xyz, d_normals4, n, p, bp, nullptr, n_vertices, n_faces, stats);
}
extern "C" int rsm_poisson_mesh_banded_weighted(rsm_ctx *c, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p, const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp, int64_t *n_vertices,
    int64_t *n_faces, double *stats) {
    return poisson_mesh_entry(c, PoissonCall{true, true}, false, xyz, normals4, n, p, bp, dp, n_vertices, n_faces, stats);
}
extern "C" int rsm_poisson_mesh_banded_weighted_device(rsm_ctx *c, const float *d_xyz, const float *d_normals4, int64_t n, const rsm_poisson_params *p, const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp, int64_t *n_vertices,
    int64_t *n_faces, double *stats) {
    return poisson_mesh_entry(c, PoissonCall{true, true}, true, d_xyz, d_normals4, n, p, bp, dp, n_vertices, n_faces, stats);
}

static int pmesh_copy_out(rsm_ctx *c, float *xyz, int32_t *faces, hipMemcpyKind kind) {
    if (!c) return RSM_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (xyz && c->pmesh.nv > 0) HIPCHK(c, hipMemcpyAsync(xyz, c->pmesh.d_v, sizeof(float) * 3 * (size_t)c->pmesh.nv, kind, c->stream));
    if (faces && c->pmesh.nf > 0) HIPCHK(c, hipMemcpyAsync(faces, c->pmesh.d_f, sizeof(int32_t) * 3 * (size_t)c->pmesh.nf, kind, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RSM_OK;
}
extern "C" int rsm_poisson_last_mesh_device(rsm_ctx *c, float *d_xyz, int32_t *d_faces) { return pmesh_copy_out(c, d_xyz, d_faces, hipMemcpyDeviceToDevice); }
extern "C" int rsm_poisson_last_mesh(rsm_ctx *c, float *xyz, int32_t *faces) { return pmesh_copy_out(c, xyz, faces, hipMemcpyDeviceToHost); }

// ---- the stage entries of the tests (host buffers) ---------------------------------------------------------------------------------------------
// rsm_stage_poisson_rhs and, with dp, _rhs_weighted (depth_in, rho, w, d are its own)
static int stage_poisson_rhs(rsm_ctx *c, bool density, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                             const rsm_poisson_density_params *dp, const double *depth_in, double grid[4], double *b, uint8_t *occ, int64_t counts[2], double *rho,
                             double *w, double *d) {
    if (!c) return RSM_E_INVALID;
    int s = poisson_call_ok(c, PoissonCall{false, density}, p, nullptr, dp, n, nullptr);
    if (s != RSM_OK) return s;
    if (!grid || !b || !occ || !counts || (n > 0 && (!xyz || !normals4))) return set_err(c, RSM_E_INVALID, "poisson: a NULL pointer");
    if (density && (s = poisson_depth_in_ok(c, depth_in, n)) != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N3 = (size_t)1 << (3 * p->depth);
    Tmp T(c);
    float *dx = T.up(xyz, 3 * (size_t)n), *dn = T.up(normals4, 4 * (size_t)n);
    double *dd_in = depth_in ? T.up(depth_in, (size_t)n) : nullptr;
    double *db = T.alloc<double>(N3);
    DensityBufs D;
    const bool have_d = !density || D.alloc(T, n, p->depth, false);
    uint8_t *docc = T.alloc<uint8_t>(N3);
    if (!dx || !dn || (depth_in && !dd_in) || !db || !docc || !have_d) return set_err(c, RSM_E_NOMEM, "poisson: no device memory");
    if (n > 0 && (s = finish(c, T)) != RSM_OK) return s;
    if ((s = poisson_grid_device(dx, dn, n, p->depth, p->scale, grid, counts, c->stream)) != RSM_OK) return poisson_fail(c, s, "bounding box");
    if (!(grid[3] > 0.0)) {
        memset(b, 0, sizeof(double) * N3);
        memset(occ, 0, N3);
        for (double *out : {rho, w, d})
            if (out && n > 0) memset(out, 0, sizeof(double) * (size_t)n);
        return RSM_OK;
    }
    if (!density) {
        if ((s = poisson_rhs_device(dx, dn, n, p->depth, grid, nullptr, db, docc, c->stream)) != RSM_OK) return poisson_fail(c, s, "right-hand side");
    } else {
        double sample_stats[3];
        if ((s = poisson_density_rhs_device(dx, dn, n, p->depth, grid, density_kernel_depth(p, dp), dp->samples_per_node, dd_in, nullptr, db, docc, D.rho, D.w, D.d,
                                            sample_stats, c->stream)) != RSM_OK)
            return poisson_fail(c, s, "density-adaptive right-hand side");
    }
    T.later(b, db, N3).later(occ, docc, N3);
    if (density) T.later(rho, (const double *)D.rho, (size_t)n).later(w, (const double *)D.w, (size_t)n).later(d, (const double *)D.d, (size_t)n);
    return finish(c, T);
}
extern "C" int rsm_stage_poisson_rhs(rsm_ctx *c, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p, double grid[4],
                                     double *b, uint8_t *occ, int64_t counts[2]) {
    return stage_poisson_rhs(c, false, xyz, normals4, n, p, nullptr, nullptr, grid, b, occ, counts, nullptr, nullptr, nullptr);
}
extern "C" int rsm_stage_poisson_rhs_weighted(rsm_ctx *c, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                                              const rsm_poisson_density_params *dp, const double *depth_in, double grid[4], double *b, uint8_t *occ,
                                              int64_t counts[2], double *rho, double *w, double *d) {
    return stage_poisson_rhs(c, true, xyz, normals4, n, p, dp, depth_in, grid, b, occ, counts, rho, w, d);
}

extern "C" int rsm_stage_poisson_solve(rsm_ctx *c, const float *b, int depth, double rel_residual, int max_cycles, float *chi, double *residual,
                                       int *cycles, double *history) {
    if (!c) return RSM_E_INVALID;
    const rsm_poisson_params p{depth, 1.0, rel_residual, max_cycles, 0};
    int s = poisson_params_ok(c, &p);
    if (s != RSM_OK) return s;
    if (!b || !chi || !residual || !cycles) return set_err(c, RSM_E_INVALID, "poisson: a NULL pointer");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N3 = (size_t)1 << (3 * depth);
    Tmp T(c);
    float *db = T.up(b, N3), *dchi = T.alloc<float>(N3);
    if (!db || !dchi) return set_err(c, RSM_E_NOMEM, "poisson: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    s = poisson_solve_device(db, depth, rel_residual, max_cycles, dchi, residual, cycles, history, c->stream);
    if (s < 0) return poisson_fail(c, s, "solve");
    T.later(chi, dchi, N3);
    const int d = finish(c, T);
    return d != RSM_OK ? d : s;
}

extern "C" int rsm_stage_iso_mesh(rsm_ctx *c, const float *chi, int depth, double iso, const double grid[4], const uint8_t *occ, int trim_cells,
                                  int64_t *n_vertices, int64_t *n_faces) {
    if (!c) return RSM_E_INVALID;
    const rsm_poisson_params p{depth, 1.0, 0.5, 1, trim_cells};
    int s = poisson_params_ok(c, &p);
    if (s != RSM_OK) return s;
    if (!chi || !grid || !n_vertices || !n_faces || (trim_cells > 0 && !occ)) return set_err(c, RSM_E_INVALID, "poisson: a NULL pointer");
    if (!std::isfinite(iso) || !std::isfinite(grid[0]) || !std::isfinite(grid[1]) || !std::isfinite(grid[2]) || !(grid[3] > 0.0) || !std::isfinite(grid[3]))
        return set_err(c, RSM_E_INVALID, "poisson: iso or grid not finite, or h <= 0");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N3 = (size_t)1 << (3 * depth);
    Tmp T(c);
    float *dchi = T.up(chi, N3);
    uint8_t *docc = occ ? T.up(occ, N3) : nullptr;
    if (!dchi || (occ && !docc)) return set_err(c, RSM_E_NOMEM, "poisson: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int64_t un[2];
    s = poisson_extract_device(dchi, depth, iso, grid, docc, trim_cells, &c->pmesh, un, c->stream);
    mesh_replaced(c); // (also when it failed: the extraction frees the mesh before anything else)
    if (s != RSM_OK) return poisson_fail(c, s, "extraction");
    *n_vertices = c->pmesh.nv;
    *n_faces = c->pmesh.nf;
    return RSM_OK;
}

// rsm_stage_poisson_band_rhs and, with dp, _band_rhs_weighted (depth_in, rho, w, d are its own)
static int stage_poisson_band_rhs(rsm_ctx *c, bool density, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                                  const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp, const double *depth_in, const float *chi_c,
                                  int64_t max_bricks, int64_t brick_room, double grid[4], int32_t *bricks, double *b, uint8_t *occ, float *g, int64_t counts[4],
                                  double *rho, double *w, double *d) {
    if (!c) return RSM_E_INVALID;
    rsm_poisson_params coarse;
    int s = poisson_call_ok(c, PoissonCall{true, density}, p, bp, dp, n, &coarse);
    if (s != RSM_OK) return s;
    if (max_bricks < 0 || max_bricks > RSM_POISSON_BAND_MAX_BRICKS) return set_err(c, RSM_E_INVALID, "poisson: max_bricks %lld outside 0..2^20", (long long)max_bricks);
    if (brick_room < 0) return set_err(c, RSM_E_INVALID, "poisson: brick_room %lld < 0", (long long)brick_room);
    if (!grid || !bricks || !b || !occ || !g || !counts || (n > 0 && (!xyz || !normals4))) return set_err(c, RSM_E_INVALID, "poisson: a NULL pointer");
    if (density && (s = poisson_depth_in_ok(c, depth_in, n)) != RSM_OK) return s;
    if (max_bricks == 0) max_bricks = RSM_POISSON_BAND_MAX_BRICKS;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t C3 = (size_t)1 << (3 * coarse.depth);
    Tmp T(c);
    float *dx = T.up(xyz, 3 * (size_t)n), *dn = T.up(normals4, 4 * (size_t)n);
    double *dd_in = depth_in ? T.up(depth_in, (size_t)n) : nullptr;
    float *dchic = chi_c ? T.up(chi_c, C3) : T.alloc<float>(C3);
    DensityBufs D;
    if ((density && !D.alloc(T, n, p->depth, true)) || !dx || !dn || (depth_in && !dd_in) || !dchic) return set_err(c, RSM_E_NOMEM, "poisson: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    int64_t vc[2];
    if ((s = poisson_grid_device(dx, dn, n, p->depth, p->scale, grid, vc, c->stream)) != RSM_OK) return poisson_fail(c, s, "bounding box");
    counts[0] = vc[0];
    counts[1] = vc[1];
    counts[2] = counts[3] = 0;
    for (double *out : {rho, w, d})
        if (out && n > 0) memset(out, 0, sizeof(double) * (size_t)n);
    if (!(grid[3] > 0.0)) return RSM_OK;
    BandOwner band;
    if ((s = poisson_band_bricks_device(dx, dn, n, p->depth, grid, bp->band_bricks, max_bricks, &band.b, c->stream)) != RSM_OK) return poisson_fail(c, s, "bricks");
    if ((s = poisson_band_cap(c, band.b, max_bricks)) != RSM_OK) return s;
    if (band.b.n_active > brick_room)
        return set_err(c, RSM_E_INVALID, "poisson: %lld active bricks, brick_room %lld", (long long)band.b.n_active, (long long)brick_room);
    counts[2] = band.b.n_active;
    counts[3] = band.b.n_occupied;
    const size_t S = (size_t)band.b.n_active, nodes = S * 512;
    double *db = T.alloc<double>(nodes);
    uint8_t *docc = T.alloc<uint8_t>(nodes);
    float *dg = T.alloc<float>(nodes);
    if (!db || !docc || !dg) return set_err(c, RSM_E_NOMEM, "poisson: no device memory");
    double sample_stats[3];
    if (density && (s = poisson_density_samples_device(dx, dn, n, p->depth, grid, density_kernel_depth(p, dp), dp->samples_per_node, dd_in, D.rho, D.w, D.d, sample_stats,
                                                       c->stream)) != RSM_OK)
        return poisson_fail(c, s, "sample densities");
    int solved = RSM_OK;
    if (!chi_c) {
        double cres;
        int ccycles;
        if ((solved = poisson_band_coarse(c, dx, dn, n, &coarse, grid, density ? &D : nullptr, dchic, &cres, &ccycles)) < 0) return solved;
    }
    s = density ? poisson_band_density_rhs_device(band.b, dx, dn, n, grid, D.w, D.d, D.levels, nullptr, db, docc, c->stream)
                : poisson_band_rhs_device(band.b, dx, dn, n, grid, nullptr, db, docc, c->stream);
    if (s != RSM_OK) return poisson_fail(c, s, "band right-hand side");
    if ((s = poisson_band_guess_device(band.b, dchic, dg, c->stream)) != RSM_OK) return poisson_fail(c, s, "guess");
    T.later(bricks, (const int32_t *)band.b.d_active, S).later(b, (const double *)db, nodes).later(occ, (const uint8_t *)docc, nodes).later(g, (const float *)dg, nodes);
    if (density) T.later(rho, (const double *)D.rho, (size_t)n).later(w, (const double *)D.w, (size_t)n).later(d, (const double *)D.d, (size_t)n);
    s = finish(c, T);
    return s != RSM_OK ? s : solved;
}
extern "C" int rsm_stage_poisson_band_rhs(rsm_ctx *c, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                                          const rsm_poisson_band_params *bp, const float *chi_c, int64_t max_bricks, int64_t brick_room, double grid[4],
                                          int32_t *bricks, double *b, uint8_t *occ, float *g, int64_t counts[4]) {
    return stage_poisson_band_rhs(c, false, xyz, normals4, n, p, bp, nullptr, nullptr, chi_c, max_bricks, brick_room, grid, bricks, b, occ, g, counts, nullptr, nullptr,
                                  nullptr);
}
extern "C" int rsm_stage_poisson_band_rhs_weighted(rsm_ctx *c, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                                                   const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp, const double *depth_in, const float *chi_c,
                                                   int64_t max_bricks, int64_t brick_room, double grid[4], int32_t *bricks, double *b, uint8_t *occ, float *g,
                                                   int64_t counts[4], double *rho, double *w, double *d) {
    return stage_poisson_band_rhs(c, true, xyz, normals4, n, p, bp, dp, depth_in, chi_c, max_bricks, brick_room, grid, bricks, b, occ, g, counts, rho, w, d);
}

extern "C" int rsm_stage_poisson_band_solve(rsm_ctx *c, const int32_t *bricks, int64_t n_bricks, int depth, const float *b, const float *g, const float *chi_c,
                                            double rel_residual, int max_iterations, float *chi, double *residual, int *iterations, double *residual0,
                                            double *history) {
    if (!c) return RSM_E_INVALID;
    int s = poisson_band_list_ok(c, bricks, n_bricks, depth);
    if (s != RSM_OK) return s;
    if (!(rel_residual > 0.0 && rel_residual < 1.0)) return set_err(c, RSM_E_INVALID, "poisson: rel_residual %g not in (0, 1)", rel_residual);
    if (max_iterations < 1) return set_err(c, RSM_E_INVALID, "poisson: max_iterations %d < 1", max_iterations);
    if (!residual || !iterations || !residual0 || (n_bricks > 0 && (!b || !g || !chi))) return set_err(c, RSM_E_INVALID, "poisson: a NULL pointer");
    *residual = *residual0 = 0.0;
    *iterations = 0;
    if (n_bricks == 0) return RSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nodes = (size_t)n_bricks * 512;
    Tmp T(c);
    float *db = T.up(b, nodes), *dchi = T.up(g, nodes), *dchic = chi_c ? T.up(chi_c, (size_t)1 << (3 * (depth - 1))) : nullptr;
    if (!db || !dchi || (chi_c && !dchic)) return set_err(c, RSM_E_NOMEM, "poisson: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    BandOwner band;
    if ((s = poisson_band_of_list_device(bricks, n_bricks, depth, &band.b, c->stream)) != RSM_OK) return poisson_fail(c, s, "bricks");
    s = poisson_band_solve_device(band.b, db, dchic, rel_residual, max_iterations, dchi, residual0, residual, iterations, history, c->stream);
    if (s < 0) return poisson_fail(c, s, "band solve");
    T.later(chi, (const float *)dchi, nodes);
    const int d = finish(c, T);
    return d != RSM_OK ? d : s;
}

extern "C" int rsm_stage_band_iso_mesh(rsm_ctx *c, const int32_t *bricks, int64_t n_bricks, int depth, const float *chi, double iso, const double grid[4],
                                       const uint8_t *occ, int trim_cells, int64_t *n_vertices, int64_t *n_faces) {
    if (!c) return RSM_E_INVALID;
    int s = poisson_band_list_ok(c, bricks, n_bricks, depth);
    if (s != RSM_OK) return s;
    if (trim_cells < 0) return set_err(c, RSM_E_INVALID, "poisson: trim_cells %d < 0", trim_cells);
    if (!grid || !n_vertices || !n_faces || (n_bricks > 0 && !chi) || (trim_cells > 0 && !occ)) return set_err(c, RSM_E_INVALID, "poisson: a NULL pointer");
    if (!std::isfinite(iso) || !std::isfinite(grid[0]) || !std::isfinite(grid[1]) || !std::isfinite(grid[2]) || !(grid[3] > 0.0) || !std::isfinite(grid[3]))
        return set_err(c, RSM_E_INVALID, "poisson: iso or grid not finite, or h <= 0");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nodes = (size_t)n_bricks * 512;
    Tmp T(c);
    float *dchi = T.up(chi, nodes);
    uint8_t *docc = occ ? T.up(occ, nodes) : nullptr;
    if (!dchi || (occ && !docc)) return set_err(c, RSM_E_NOMEM, "poisson: no device memory");
    if ((s = finish(c, T)) != RSM_OK) return s;
    BandOwner band;
    if ((s = poisson_band_of_list_device(bricks, n_bricks, depth, &band.b, c->stream)) != RSM_OK) return poisson_fail(c, s, "bricks");
    int64_t un[2];
    s = poisson_band_extract_device(band.b, dchi, iso, grid, docc, trim_cells, &c->pmesh, un, c->stream);
    mesh_replaced(c); // (also when it failed: the extraction frees the mesh before anything else)
    if (s != RSM_OK) return poisson_fail(c, s, "extraction");
    *n_vertices = c->pmesh.nv;
    *n_faces = c->pmesh.nf;
    return RSM_OK;
}
