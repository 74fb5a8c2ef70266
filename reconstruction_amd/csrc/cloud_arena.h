// cloud_arena.h -- the scratch arena of the cloud steps (k_filter.hip, k_mls.hip, k_dedup.hip; rsm_cloud.hip reserves it and places their
// buffers through rsm_dev.h's filter_arena_* functions; those are defined in cloud_grid.hip).
// Grow-only device arena owned by the context: one hipMalloc sized for the cloud at hand instead of ~25 hipMalloc / hipFree pairs per
// call (hipFree synchronises the device).  Stack discipline: a step notes `off` and sets it back when its buffers are done.
#pragma once

#include "rsm_dev.h"

// k_filter.hip's k_dist_stats: the sums of the per-point distances and what proves them exact
struct DistStats {
    double sum, sq_sum;
    int q_sum, q_sq;
    int bad; // a NaN distance, or one whose float32 square is not finite (a point beyond 1.8e19: its neighbours' squared distances overflow);
             // makes the host take the sequential path
};

#define FA_SAMPLES 8192
// the arena's small pinned host block: where each step's copies from the device land
struct FilterPinned {
    float samples[3 * FA_SAMPLES]; // sample_extent: the points the robust extent is taken from
    unsigned int bb[8];            // cloud_bbox: ord(min) x 3, ord(max) x 3, the finite points
    int cnt[4];                    // the filter: [0..2] a list's length / the probe's counters / a compaction's total, [3] the normals' widest window
    DistStats stats;               // the filter's distance statistics
    alignas(8) unsigned char caller[64]; // filter_arena_host: free for the step that holds the arena (k_mls.hip's and k_dedup.hip's totals)
};

struct FilterArena {
    char *base = nullptr;
    size_t cap = 0, off = 0;
    FilterPinned *pin = nullptr;
    bool failed = false;
    template <typename T>
    T *get(size_t n) {
        const size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
        if (off + bytes > cap) {
            failed = true;
            return nullptr;
        }
        T *p = (T *)(base + off);
        off += bytes;
        return p;
    }
};
