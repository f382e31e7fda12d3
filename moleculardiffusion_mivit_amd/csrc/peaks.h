// Peak selection on a per-pixel map of a movie, shared by the difference-of-Gaussians detector (csrc/tracking.hip) and the
// likelihood-ratio detector (csrc/detect.hip): per-frame keys, the local-maximum mask and the sorted greedy spacing pass.
// The map kernel of each detector sits between tk_init_kernel and tk_mask_kernel and leaves the frame's max / min keys.
//
//   tk_init_kernel    per frame: max / min keys and the candidate counter.
//   tk_mask_kernel    one thread per pixel: above the threshold and not exceeded by any pixel of its (2 min_distance + 1)^2
//                     window (replicated borders add no new value, so the window is just clipped) -> appended to the frame's
//                     candidate list through its counter as a 64-bit key.  A frame with min == max (every pixel a window
//                     maximum) has no candidate.  The threshold is threshold * max of the frame (one fp32 product), or with
//                     absolute != 0 the threshold itself.
//   tk_select_kernel  one workgroup per frame: bitonic sort of the keys in LDS, then the greedy spacing pass.  The key is
//                     (inverted ordered value, row-major index), so the sort alone defines the order (value descending, ties
//                     by index ascending) whatever order the atomics appended in.
// Each translation unit that includes this gets its own copy of the kernels (anonymous namespace, no relocatable device code).
#pragma once

#include "common.h"

namespace {

constexpr int TK_TX = 64, TK_TY = 16; // tile of one workgroup (256 threads)
constexpr int TK_MAX_MIN_DISTANCE = 16;
constexpr int TK_MAX_CAP = 2048;      // candidates per frame: 8-byte keys + kept (y, x) in LDS, 32 KiB

// float <-> int whose signed order is the float order (no NaN in a filtered finite movie)
__device__ __forceinline__ int ordered_key(float v) {
    const int i = __float_as_int(v);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ordered_value(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__global__ __launch_bounds__(256) void tk_init_kernel(int *maxkey, int *minkey, int *ncand, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    maxkey[f] = INT32_MIN;
    minkey[f] = INT32_MAX;
    ncand[f] = 0;
}

__global__ __launch_bounds__(256) void tk_mask_kernel(const float *__restrict__ dog, const int *__restrict__ maxkey,
                                                      const int *__restrict__ minkey, int *ncand,
                                                      unsigned long long *cand, int64_t total, int H, int W, int m, int cap,
                                                      float threshold, int absolute) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const int HW = H * W;
    const int f = (int)(p / HW), idx = (int)(p - (int64_t)f * HW);
    const int mk = maxkey[f];
    if (mk == minkey[f]) return;                                          // flat frame: every pixel is a maximum -> none
    const float thr = absolute ? threshold : threshold * ordered_value(mk);
    const float *d = dog + (int64_t)f * HW;
    const float v = d[idx];
    if (!(v > thr)) return;
    const int y = idx / W, x = idx - y * W;
    const int ya = y - m < 0 ? 0 : y - m, yb = y + m > H - 1 ? H - 1 : y + m;
    const int xa = x - m < 0 ? 0 : x - m, xb = x + m > W - 1 ? W - 1 : x + m;
    for (int yy = ya; yy <= yb; ++yy)
        for (int xx = xa; xx <= xb; ++xx)
            if (d[yy * W + xx] > v) return;
    const int slot = atomicAdd(ncand + f, 1);
    if (slot >= cap) return;                                              // counted, reported, never stored out of bounds
    const unsigned hi = ~((unsigned)ordered_key(v) ^ 0x80000000u);        // larger value -> smaller key
    cand[(int64_t)f * cap + slot] = ((unsigned long long)hi << 32) | (unsigned)idx;
}

__global__ __launch_bounds__(256) void tk_select_kernel(const unsigned long long *__restrict__ cand,
                                                        const int *__restrict__ ncand, int W, int m, int cap, int n2max,
                                                        int *count, int *coords, float *values) {
    extern __shared__ unsigned long long tk_keys[];                       // n2max keys, then cap kept (y, x) pairs
    __shared__ int nkept;
    int *kept = reinterpret_cast<int *>(tk_keys + n2max);
    const int f = blockIdx.x;
    const int nc = ncand[f];
    const int n = nc < cap ? nc : cap;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = threadIdx.x; i < n2; i += blockDim.x) tk_keys[i] = i < n ? cand[(int64_t)f * cap + i] : ~0ull;
    if (threadIdx.x == 0) nkept = 0;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += blockDim.x) {
                const int o = i ^ j;
                if (o > i) {
                    const unsigned long long x = tk_keys[i], y = tk_keys[o];
                    if ((x > y) == ((i & k) == 0)) {
                        tk_keys[i] = y;
                        tk_keys[o] = x;
                    }
                }
            }
            __syncthreads();
        }
    // greedy spacing in sorted order: keep a candidate unless a kept one lies within Chebyshev distance m
    for (int i = 0; i < n; ++i) {
        const unsigned long long key = tk_keys[i];
        const int idx = (int)(unsigned)(key & 0xffffffffu);
        const int y = idx / W, x = idx - y * W;
        const int nk = nkept;
        int clash = 0;
        for (int j = threadIdx.x; j < nk; j += blockDim.x) {
            const int dy = kept[2 * j] - y, dx = kept[2 * j + 1] - x;
            if ((dy < 0 ? -dy : dy) <= m && (dx < 0 ? -dx : dx) <= m) clash = 1;
        }
        clash = __syncthreads_or(clash);
        if (!clash && threadIdx.x == 0) {
            kept[2 * nk] = y;
            kept[2 * nk + 1] = x;
            coords[((int64_t)f * cap + nk) * 2] = y;
            coords[((int64_t)f * cap + nk) * 2 + 1] = x;
            values[(int64_t)f * cap + nk] = ordered_value((int)(~(unsigned)(key >> 32) ^ 0x80000000u));
            nkept = nk + 1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) count[f] = nkept;
}

inline int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace
