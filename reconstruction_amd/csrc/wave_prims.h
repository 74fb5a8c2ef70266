// wave_prims.h -- what the kernels share on the device at the width of one wave (64 lanes): reductions into every lane, the lane masks
// that go with a ballot, and inclusive scans along the lanes.  Device side and header only (dev_prims.h is the host plumbing).
#pragma once

// a value of every lane reduced over the wave, into every lane
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, const Op &op) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    return wave_reduce(v, [](T a, T b) { return a + b; });
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
    return wave_reduce(v, [](T a, T b) { return min(a, b); });
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
    return wave_reduce(v, [](T a, T b) { return max(a, b); });
}

// ballot masks: the lanes below `lane`, those up to and including it, those from it on
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ unsigned long long lanes_upto(int lane) { return (2ull << lane) - 1ull; }
__device__ __forceinline__ unsigned long long lanes_from(int lane) { return ~lanes_below(lane); }
// the position of `lane` among the set lanes of a ballot: where it writes when the set lanes compact in lane order
__device__ __forceinline__ int ballot_rank(unsigned long long mask, int lane) { return __popcll(mask & lanes_below(lane)); }

// the value of the lane s before this one in scan order: s below it for an upward scan, s above it for a downward one (its own
// where the wave has no such lane)
template <bool UP, class T>
__device__ __forceinline__ T wave_prev(T v, int s = 1) {
    return UP ? __shfl_up(v, s) : __shfl_down(v, s);
}
// Inclusive scan under op along the lanes: an upward scan leaves op over lanes head .. lane in `lane`, a downward one op over lanes
// lane .. head.  Without `head` the whole wave is one segment; with it the scan is segmented: `head` is the lane's own bound (head <= lane
// upward, head >= lane downward), the same in every lane of a segment.  A scan that runs on through several waves' worth of elements
// keeps its carry in the caller.
template <bool UP, class T, class Op>
__device__ __forceinline__ T wave_scan(T v, int lane, const Op &op, int head = UP ? 0 : 63) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const T o = wave_prev<UP>(v, s);
        if (UP ? lane - s >= head : lane + s <= head) v = op(v, o);
    }
    return v;
}
