// Stage drift: the per-frame statistic of the frame-to-frame increments of all tracks (mean or exact median), the windowed
// velocity and its running sum (trackpy's compute_drift; no counterpart in the reference, whose movies do not drift).
// include/mivit_hip.h spells the arithmetic and every summation order out; helpers/msd.py restates them in numpy, bitwise.
//
// mivit_drift_frames, one launch: ONE WORKGROUP of 256 threads per frame.  The workgroup gathers the frame's increments
// pos[r] - pos[r - 1] itself (r from pair_row, the frame's slice from frame_offsets).
//   mean:   thread t sums the increments at the positions t, t + 256, ... of the frame in ascending position, starting from
//           +0; the 256 partial sums go through LDS and are folded in halves (128, 64, .. 1: entry i takes entry i + half).
//           The order is a function of the increment's position in its frame alone.  No limit on the pairs of a frame.
//   median: the increments of one axis at a time become 64-bit keys whose unsigned order is the order of the values with -0
//           before +0, padded to a power of two with the largest key, and a bitonic network sorts them in LDS (8 B a pair:
//           DRIFT_MAX_PAIRS = 4096 pairs are 32 KiB, five workgroups a CU; the launch sizes LDS to the largest frame of the
//           call).  The result of a sorting network does not depend on which thread ran which comparator, and the keys are
//           a total order, so the two middle values are the same bits however the frame was dealt.
// No atomics, nothing shared between frames: a frame's result is bitwise the same alone, in any batch and in every launch.
//
// mivit_drift_integrate, two launches: one thread per (frame, axis) sums its window in ascending frame; then ONE workgroup
// runs the blocked running sum: thread b sums block b of 256 frames sequentially, one thread per axis sums the block totals
// sequentially, and every entry past block 0 gets its block's offset added.  256 blocks (65 536 frames) at a time, the
// offset carried on: the order does not depend on that chunking, and drift[f] depends on velocity[0 .. f] alone.
//
// No contraction into FMA, as in diffusion.hip: n * stat + sum must round twice, as numpy does.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int DRIFT_THREADS = 256;
constexpr int DRIFT_MAX_PAIRS = 4096;     // ops.DRIFT_MAX_PAIRS: pairs of a frame the median sorts in LDS (8 B a pair)
constexpr int SCAN_BLOCK = 256;           // frames a thread sums sequentially in the running sum (msd._DRIFT_SCAN_BLOCK)

__host__ __device__ constexpr int drift_pow2(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// the unsigned order of the keys is the order of the values, -0 before +0 (NaN is kept out by the caller)
__device__ __forceinline__ unsigned long long drift_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double drift_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

__global__ __launch_bounds__(DRIFT_THREADS) void drift_frames_kernel(const double *__restrict__ pos, int N,
                                                                     const int *__restrict__ pair_row, int M,
                                                                     const int *__restrict__ frame_offsets, int mode,
                                                                     int lds_pairs, double *__restrict__ stat) {
    extern __shared__ double drift_lds[];                                 // max(lds_pairs, DRIFT_THREADS) entries of 8 B
    const int f = blockIdx.x, t = threadIdx.x;
    int a = frame_offsets[f], b = frame_offsets[f + 1];
    a = a < 0 ? 0 : (a > M ? M : a);                                      // never read outside pair_row, whatever the CSR holds
    b = b < a ? a : (b > M ? M : b);
    int n = b - a;
    if (n == 0 || N < 2) {                                                // uniform over the workgroup
        if (t < 2) stat[2 * f + t] = 0.0;
        return;
    }
    if (mode == 0) {
        double sy = 0.0, sx = 0.0;
        for (int i = t; i < n; i += DRIFT_THREADS) {
            int r = pair_row[a + i];
            r = r < 1 ? 1 : (r > N - 1 ? N - 1 : r);                      // never read outside pos
            const double *q = pos + (int64_t)r * 2;
            sy = sy + (q[0] - q[-2]);
            sx = sx + (q[1] - q[-1]);
        }
        for (int axis = 0; axis < 2; ++axis) {
            drift_lds[t] = axis == 0 ? sy : sx;
            __syncthreads();
            for (int half = DRIFT_THREADS / 2; half > 0; half >>= 1) {
                if (t < half) drift_lds[t] = drift_lds[t] + drift_lds[t + half];
                __syncthreads();
            }
            if (t == 0) stat[2 * f + axis] = drift_lds[0] / (double)n;
            __syncthreads();
        }
        return;
    }
    if (n > lds_pairs) n = lds_pairs;                                     // never write outside LDS (the host checked)
    const int P = drift_pow2(n);                                          // <= lds_pairs: the host passes a power of two
    unsigned long long *key = reinterpret_cast<unsigned long long *>(drift_lds);
    for (int axis = 0; axis < 2; ++axis) {
        int bad = 0;
        for (int i = t; i < P; i += DRIFT_THREADS) {
            unsigned long long k = ~0ull;                                 // the padding sorts last
            if (i < n) {
                int r = pair_row[a + i];
                r = r < 1 ? 1 : (r > N - 1 ? N - 1 : r);
                const double d = pos[(int64_t)r * 2 + axis] - pos[(int64_t)(r - 1) * 2 + axis];
                if (d != d) bad = 1;
                k = drift_key(d);
            }
            key[i] = k;
        }
        bad = __syncthreads_or(bad);                                      // also the barrier between the fill and the sort
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int c = t; c < (P >> 1); c += DRIFT_THREADS) {
                    const int lo = 2 * c - (c & (stride - 1));            // the comparator's lower index; its partner lo + stride
                    const bool up = (lo & size) == 0;
                    const unsigned long long x = key[lo], y = key[lo + stride];
                    if ((x > y) == up) {
                        key[lo] = y;
                        key[lo + stride] = x;
                    }
                }
                __syncthreads();
            }
        }
        if (t == 0) {
            double m;
            if (bad) {
                m = NAN;                                                  // np.median of a frame with a NaN
            } else if (n & 1) {
                m = drift_unkey(key[n >> 1]);
            } else {
                m = (drift_unkey(key[(n >> 1) - 1]) + drift_unkey(key[n >> 1])) / 2.0;
            }
            stat[2 * f + axis] = m;
        }
        __syncthreads();                                                  // the keys are read before the next axis overwrites them
    }
}

__global__ __launch_bounds__(DRIFT_THREADS) void drift_velocity_kernel(const double *__restrict__ stat,
                                                                       const int *__restrict__ n_pairs, int F, int h,
                                                                       double *__restrict__ velocity) {
    const int64_t i = (int64_t)blockIdx.x * DRIFT_THREADS + threadIdx.x;
    if (i >= (int64_t)F * 2) return;
    const int f = (int)(i >> 1), axis = (int)(i & 1);
    double v = 0.0;
    if (f >= 1) {
        if (h == 0) {
            v = stat[i];
        } else {
            const int g0 = f - h < 1 ? 1 : f - h;                         // f - h cannot wrap: h <= F
            const int g1 = (int64_t)f + h > F - 1 ? F - 1 : f + h;
            double num = 0.0;
            int64_t den = 0;
            for (int g = g0; g <= g1; ++g) {
                const int c = n_pairs[g] > 0 ? n_pairs[g] : 0;
                num = num + (double)c * stat[2 * (int64_t)g + axis];
                den += c;
            }
            v = den > 0 ? num / (double)den : 0.0;
        }
    }
    velocity[i] = v;
}

__global__ __launch_bounds__(SCAN_BLOCK) void drift_scan_kernel(const double *__restrict__ velocity, int F,
                                                                double *__restrict__ drift) {
    __shared__ double tot[SCAN_BLOCK][2];                                 // block totals, then block offsets
    const int t = threadIdx.x;
    const int n_blocks = (F + SCAN_BLOCK - 1) / SCAN_BLOCK;
    double carry = 0.0;                                                   // threads 0 / 1: the sum of all earlier block totals
    for (int b0 = 0; b0 < n_blocks; b0 += SCAN_BLOCK) {
        const int blk = b0 + t;
        const int64_t f0 = (int64_t)blk * SCAN_BLOCK;
        const int len = blk < n_blocks ? (int)(F - f0 < SCAN_BLOCK ? F - f0 : SCAN_BLOCK) : 0;
        double ry = 0.0, rx = 0.0;
        for (int i = 0; i < len; ++i) {
            const double vy = velocity[2 * (f0 + i)], vx = velocity[2 * (f0 + i) + 1];
            ry = i == 0 ? vy : ry + vy;                                   // np.cumsum: the first entry is itself
            rx = i == 0 ? vx : rx + vx;
            drift[2 * (f0 + i)] = ry;
            drift[2 * (f0 + i) + 1] = rx;
        }
        tot[t][0] = ry;
        tot[t][1] = rx;
        __syncthreads();
        if (t < 2) {
            for (int j = 0; j < SCAN_BLOCK && b0 + j < n_blocks; ++j) {   // sequential over the blocks, ascending
                const double own = tot[j][t];
                tot[j][t] = carry;                                        // the offset of block b0 + j
                carry = (b0 + j == 0) ? own : carry + own;
            }
        }
        __syncthreads();
        if (blk >= 1) {                                                   // block 0 has no offset: its entries stay as summed
            const double oy = tot[t][0], ox = tot[t][1];
            for (int i = 0; i < len; ++i) {                               // a thread rereads only what it wrote itself
                drift[2 * (f0 + i)] = oy + drift[2 * (f0 + i)];
                drift[2 * (f0 + i) + 1] = ox + drift[2 * (f0 + i) + 1];
            }
        }
        __syncthreads();                                                  // tot is reused by the next 256 blocks
    }
}

}  // namespace

extern "C" int mivit_drift_frames(const double *pos, int N, const int *pair_row, int M, const int *frame_offsets, int F,
                                  int mode, int max_pairs, double *stat, void *stream) {
    MIVIT_CHECK(N >= 0 && M >= 0 && F >= 0, "drift_frames: N = %d, M = %d, F = %d: negative size", N, M, F);
    MIVIT_CHECK(mode == 0 || mode == 1, "drift_frames: mode = %d, 0 (mean) and 1 (median) exist", mode);
    MIVIT_CHECK(max_pairs >= 0 && max_pairs <= M, "drift_frames: max_pairs = %d outside 0 .. M = %d", max_pairs, M);
    MIVIT_CHECK(mode == 0 || max_pairs <= DRIFT_MAX_PAIRS,
                "drift_frames: a frame of %d pairs, the median's limit is %d (it sorts a frame in LDS)", max_pairs,
                DRIFT_MAX_PAIRS);
    MIVIT_CHECK(M == 0 || N >= 2, "drift_frames: %d pairs need at least 2 rows, got N = %d", M, N);
    if (F == 0) return 0;
    MIVIT_CHECK(frame_offsets && stat, "drift_frames: null pointer");
    MIVIT_CHECK((pos && pair_row) || M == 0, "drift_frames: null pointer");
    const int lds_pairs = mode == 1 ? drift_pow2(max_pairs) : 0;          // <= 4096: 32 KiB, below the 64 KiB a launch may ask for
    const size_t bytes = sizeof(double) * (size_t)(lds_pairs > DRIFT_THREADS ? lds_pairs : DRIFT_THREADS);
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(drift_frames_kernel, dim3((unsigned)F), dim3(DRIFT_THREADS), bytes, static_cast<hipStream_t>(stream), pos,
                       N, pair_row, M, frame_offsets, mode, lds_pairs, stat);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_drift_integrate(const double *stat, const int *n_pairs, int F, int half_window, double *velocity,
                                     double *drift, void *stream) {
    MIVIT_CHECK(F >= 0, "drift_integrate: F = %d: negative size", F);
    MIVIT_CHECK(half_window >= 0, "drift_integrate: half_window = %d must be >= 0", half_window);
    if (F == 0) return 0;
    MIVIT_CHECK(stat && n_pairs && velocity && drift, "drift_integrate: null pointer");
    const int h = half_window > F ? F : half_window;                      // a wider window sees the same frames
    prof_set_tag(MIVIT_PROF_OP);
    const int64_t n = (int64_t)F * 2;
    hipLaunchKernelGGL(drift_velocity_kernel, dim3((unsigned)((n + DRIFT_THREADS - 1) / DRIFT_THREADS)), dim3(DRIFT_THREADS), 0,
                       static_cast<hipStream_t>(stream), stat, n_pairs, F, h, velocity);
    MIVIT_LAUNCH_CHECK();
    hipLaunchKernelGGL(drift_scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, static_cast<hipStream_t>(stream), velocity, F, drift);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
