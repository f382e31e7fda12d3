// Multi-state diffusion: the state paths of a switching simulator, the optimal partition of a track into stretches of constant
// step variance, and one row of estimates per stretch (no counterpart in the reference, whose trajectories are single_state;
// the model is andi_datasets' multi_state, the estimator the covariance-based one of Vestergaard, Blainey & Flyvbjerg,
// Phys. Rev. E 89, 022726 (2014)).  include/mivit_hip.h spells the arithmetic out; helpers/msd.py and helpers/generation.py
// restate it in numpy.
//
// mivit_segment_tracks, one launch: ONE WAVE per track (a workgroup of 64 threads), the optimal-partitioning recurrence
//     F(j) = min_i F(i) + C(i, j) + beta,   C(i, j) = 2 n log(max((cs[j] - cs[i]) / (2 n), min_var)),   n = j - i
// sequential in j and parallel over the candidates i.  cs (the prefix sums of the squared increments, summed by one lane in
// ascending order: np.cumsum bit for bit), F and prev live in LDS, 20 bytes a row.  Lane l takes the candidates l, l + 64, ...
// in ascending index and keeps the first minimum; a xor butterfly over (value, index) that prefers the lower index on equal
// values leaves the same pair in every lane.  That pair is the minimum of a total order, so it does not depend on how the
// candidates were dealt: the lowest index among equal minima, as np.argmin gives it.  A workgroup of one wave needs no
// s_barrier (the compiler drops it; __syncthreads is then the LDS fence alone), which is what the many short tracks of a real
// movie want: a step of a track of up to 64 + 2 min_len increments is one pass of the wave.  No atomics, the mapping does
// not depend on the batch: a track's result is bitwise the same alone and in any batch.
//
// mivit_segment_stats, one launch: one thread per segment, sums in ascending index, no log: bitwise the numpy restatement.
// mivit_markov_states, one launch: one thread per particle walks its T uniforms; adds and compares only: bitwise as well.
//
// No contraction into FMA, as in diffusion.hip.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int SEG_THREADS = 64;       // one wave
constexpr int SEG_MAX_LEN = 4096;     // rows of a track: 20 B a row of LDS, 80 KiB (ops.SEG_MAX_LEN)
constexpr int STAT_THREADS = 256;
constexpr int MARKOV_THREADS = 64;
constexpr int MARKOV_MAX_K = 8;       // ops.MARKOV_MAX_K

__host__ __device__ constexpr size_t seg_lds_bytes(int rows) { return (size_t)rows * (2 * sizeof(double) + sizeof(int)); }

// C(i, j) of n = j - i increments whose squared lengths sum to d
__device__ __forceinline__ double seg_cost(double d, int n, double min_var) {
    const double tn = 2.0 * (double)n;
    double r = d / tn;
    r = r < min_var ? min_var : r;                                        // np.maximum: a NaN stays
    return tn * log(r);
}

__global__ __launch_bounds__(SEG_THREADS) void seg_tracks_kernel(const double *__restrict__ pos, int N,
                                                                 const int *__restrict__ offsets, int min_len, double penalty,
                                                                 double min_var, int max_len, int *__restrict__ seg_start,
                                                                 double *__restrict__ cost) {
    extern __shared__ double seg_lds[];
    double *cs = seg_lds;                                                 // [max_len]: cs[j] = q_0 + .. + q_{j-1}
    double *F = cs + max_len;                                             // [max_len]
    int *prev = reinterpret_cast<int *>(F + max_len);                     // [max_len]; the sign bit marks a changepoint
    const int k = blockIdx.x, lane = threadIdx.x;
    int a = offsets[k], b = offsets[k + 1];
    a = a < 0 ? 0 : (a > N ? N : a);                                      // never read outside pos, whatever offsets holds
    b = b < a ? a : (b > N ? N : b);
    int L = b - a;
    if (L > max_len) L = max_len;                                         // never write outside LDS (the host checked)
    const int Linc = L - 1;
    if (Linc < 1) {                                                       // uniform over the wave
        if (lane == 0) {
            if (L == 1) seg_start[a] = 1;
            cost[k] = NAN;
        }
        return;
    }
    const double *p = pos + (int64_t)a * 2;
    for (int r = lane; r < L; r += SEG_THREADS) {
        prev[r] = 0;
        if (r < Linc) {
            const double dy = p[2 * (r + 1)] - p[2 * r], dx = p[2 * (r + 1) + 1] - p[2 * r + 1];
            cs[r + 1] = dy * dy + dx * dx;
        }
    }
    __syncthreads();
    if (lane == 0) {
        double run = 0.0;
        cs[0] = 0.0;
        for (int r = 1; r <= Linc; ++r) {
            run = run + cs[r];
            cs[r] = run;
        }
    }
    __syncthreads();
    const double beta = penalty * log((double)Linc);
    double fl;
    if (Linc < min_len) {                                                 // the recurrence has no step: one segment
        fl = (-beta + seg_cost(cs[Linc], Linc, min_var)) + beta;
    } else {
        if (lane == 0) F[0] = -beta;
        __syncthreads();
        fl = 0.0;
        for (int j = min_len; j <= Linc; ++j) {
            const int ncand = 1 + (j - 2 * min_len + 1 > 0 ? j - 2 * min_len + 1 : 0);     // i = 0, then min_len .. j - min_len
            const double cj = cs[j];
            double bv = INFINITY;
            int bi = 0x7fffffff;
            for (int c = lane; c < ncand; c += SEG_THREADS) {
                const int i = c == 0 ? 0 : min_len + c - 1;
                const double v = (F[i] + seg_cost(cj - cs[i], j - i, min_var)) + beta;
                if (v < bv) {                                             // ascending i: the first minimum stays
                    bv = v;
                    bi = i;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ov < bv || (ov == bv && oi < bi)) {
                    bv = ov;
                    bi = oi;
                }
            }
            if (bi < 0 || bi >= j) bi = 0;                                // only where every candidate was NaN
            if (lane == 0) {
                F[j] = bv;
                prev[j] = bi;
            }
            fl = bv;
            __syncthreads();                                              // one wave: the LDS fence, no s_barrier
        }
    }
    if (lane == 0) {
        cost[k] = fl;
        int j = Linc;
        while (j > 0) {                                                   // i < j always: at most Linc rounds
            int i = j >= min_len ? (prev[j] & 0x7fffffff) : 0;
            if (i >= j) i = 0;
            if (i > 0) prev[i] = prev[i] | (int)0x80000000;
            j = i;
        }
    }
    __syncthreads();
    for (int r = lane; r < L; r += SEG_THREADS) seg_start[a + r] = (r == 0 || prev[r] < 0) ? 1 : 0;
}

__global__ __launch_bounds__(STAT_THREADS) void seg_stats_kernel(const double *__restrict__ pos, int N,
                                                                 const int *__restrict__ seg_offsets,
                                                                 const int *__restrict__ seg_track_end, int n_seg, double dt,
                                                                 double R, double *__restrict__ d_cve, double *__restrict__ d_mle,
                                                                 double *__restrict__ sigma2, int *__restrict__ n_inc) {
    const int s = blockIdx.x * STAT_THREADS + threadIdx.x;
    if (s >= n_seg) return;
    int r0 = seg_offsets[s], r1 = seg_offsets[s + 1];
    const int e = seg_track_end[s] - 1;
    if (r1 > e) r1 = e;                                                   // the bridging increment, unless the track ends
    if (r1 > N - 1) r1 = N - 1;                                           // never read outside pos
    if (r0 < 0) r0 = 0;
    const int n = r1 > r0 ? r1 - r0 : 0;
    double S2 = 0.0, S11 = 0.0, py = 0.0, px = 0.0;
    for (int i = 0; i < n; ++i) {
        const double *q = pos + (int64_t)(r0 + i) * 2;
        const double dy = q[2] - q[0], dx = q[3] - q[1];
        S2 = S2 + (dy * dy + dx * dx);
        if (i > 0) S11 = S11 + (py * dy + px * dx);
        py = dy;
        px = dx;
    }
    double mle = NAN, cve = NAN, sg = NAN;
    if (n >= 1) mle = S2 / ((4.0 * (double)n) * dt);
    if (n >= 2) {
        const double m1 = 2.0 * (double)(n - 1);
        cve = mle + S11 / (m1 * dt);
        sg = (R * S2) / (2.0 * (double)n) + ((2.0 * R - 1.0) * S11) / m1;
    }
    d_cve[s] = cve;
    d_mle[s] = mle;
    sigma2[s] = sg;
    n_inc[s] = n;
}

__global__ __launch_bounds__(MARKOV_THREADS) void markov_kernel(const double *__restrict__ u, const double *__restrict__ p0,
                                                                const double *__restrict__ M, int N, int T, int K,
                                                                int *__restrict__ state) {
    __shared__ double rows[(MARKOV_MAX_K + 1) * MARKOV_MAX_K];            // row 0: p0, row 1 + k: M[k]
    for (int i = threadIdx.x; i < (K + 1) * K; i += MARKOV_THREADS) rows[i] = i < K ? p0[i] : M[i - K];
    __syncthreads();
    const int n = blockIdx.x * MARKOV_THREADS + threadIdx.x;
    if (n >= N) return;
    const double *un = u + (int64_t)n * T;
    int *sn = state + (int64_t)n * T;
    int row = 0;
    for (int t = 0; t < T; ++t) {
        const double *pr = rows + row * K;
        const double ut = un[t];
        double c = pr[0];
        int k = 0;
        while (k < K - 1 && !(ut < c)) {                                  // the last state catches rounding (and a NaN)
            ++k;
            c = c + pr[k];
        }
        sn[t] = k;
        row = 1 + k;
    }
}

}  // namespace

extern "C" int mivit_segment_tracks(const double *pos, int N, const int *offsets, int n_tracks, int max_len, int min_len,
                                    double penalty, double min_var, int *seg_start, double *cost, void *stream) {
    MIVIT_CHECK(N >= 0 && n_tracks >= 0, "segment_tracks: N = %d, n_tracks = %d: negative size", N, n_tracks);
    MIVIT_CHECK(min_len >= 2, "segment_tracks: min_len = %d, a stretch needs at least 2 increments", min_len);
    MIVIT_CHECK(max_len >= 0 && max_len <= SEG_MAX_LEN,
                "segment_tracks: a track of %d rows, the limit is %d (the recurrence's state lives in LDS)", max_len, SEG_MAX_LEN);
    MIVIT_CHECK(penalty >= 0.0, "segment_tracks: penalty = %g must be >= 0", penalty);
    MIVIT_CHECK(min_var > 0.0 && min_var < INFINITY, "segment_tracks: min_var = %g must be positive and finite", min_var);
    if (n_tracks == 0) return 0;
    MIVIT_CHECK(offsets && cost, "segment_tracks: null pointer");
    MIVIT_CHECK((pos && seg_start) || N == 0, "segment_tracks: null pointer");
    const int rows = max_len < 2 ? 2 : max_len;
    const size_t bytes = seg_lds_bytes(rows);
    if (bytes > 48 * 1024)
        MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(seg_tracks_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(seg_tracks_kernel, dim3((unsigned)n_tracks), dim3(SEG_THREADS), bytes, static_cast<hipStream_t>(stream),
                       pos, N, offsets, min_len, penalty, min_var, rows, seg_start, cost);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_segment_stats(const double *pos, int N, const int *seg_offsets, const int *seg_track_end, int n_seg,
                                   double dt, double R, double *d_cve, double *d_mle, double *sigma2, int *n_increments,
                                   void *stream) {
    MIVIT_CHECK(N >= 0 && n_seg >= 0, "segment_stats: N = %d, n_seg = %d: negative size", N, n_seg);
    MIVIT_CHECK(dt > 0.0 && dt < INFINITY, "segment_stats: dt = %g must be positive and finite", dt);
    MIVIT_CHECK(R >= 0.0 && R <= 0.25, "segment_stats: blur coefficient R = %g outside [0, 1/4]", R);
    if (n_seg == 0) return 0;
    MIVIT_CHECK(seg_offsets && seg_track_end && d_cve && d_mle && sigma2 && n_increments, "segment_stats: null pointer");
    MIVIT_CHECK(pos || N == 0, "segment_stats: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(seg_stats_kernel, dim3((unsigned)ceil_div(n_seg, STAT_THREADS)), dim3(STAT_THREADS), 0,
                       static_cast<hipStream_t>(stream), pos, N, seg_offsets, seg_track_end, n_seg, dt, R, d_cve, d_mle, sigma2,
                       n_increments);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_markov_states(const double *u, const double *p0, const double *M, int N, int T, int K, int *state,
                                   void *stream) {
    MIVIT_CHECK(N >= 0 && T >= 0, "markov_states: N = %d, T = %d: negative size", N, T);
    MIVIT_CHECK(K >= 1 && K <= MARKOV_MAX_K, "markov_states: K = %d states, 1 .. %d are supported", K, MARKOV_MAX_K);
    if (N == 0 || T == 0) return 0;
    MIVIT_CHECK(u && p0 && M && state, "markov_states: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(markov_kernel, dim3((unsigned)ceil_div(N, MARKOV_THREADS)), dim3(MARKOV_THREADS), 0,
                       static_cast<hipStream_t>(stream), u, p0, M, N, T, K, state);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
