// Tracks whose motion changes: the optimal partition of a track into stretches, under two stretch models, one row of
// estimates per stretch, and the state paths of a switching simulator (no counterpart in the reference, whose trajectories
// are single_state; the multi-state model is andi_datasets' multi_state, the estimators are the covariance-based ones of
// Vestergaard, Blainey & Flyvbjerg, Phys. Rev. E 89, 022726 (2014)).  include/mivit_hip.h spells the arithmetic out;
// helpers/msd.py and helpers/generation.py restate it in numpy.
//
// mivit_segment_tracks and mivit_segment_transport, one launch of partition_kernel<Model>: ONE WAVE per track (a workgroup of
// 64 threads), the optimal-partitioning recurrence
//     F(j) = min_i F(i) + C(i, j) + beta,   n = j - i
// sequential in j and parallel over the candidates i.  A stretch model says how many prefix sums over the increments it
// needs, what an increment adds to each, how many classes of stretch it tells apart, and what C(i, j) and the class of the
// stretch are from the differences of those sums:
//     VarianceModel            one sum (dy^2 + dx^2), C = 2 n log(max(SS / (2 n), min_var)), class 0: stretches of constant step
//                              variance (mivit_segment_tracks, and mivit_segment_transport with classes = 2)
//     TransportModel<false>    three sums (dy^2 + dx^2, dy, dx): the lower of that cost (class 0, diffusive) and of the cost
//                              about a constant velocity plus gamma (class 1, directed); a tie is diffusive
//     TransportModel<true>     the same sums, directed always
// The sums (each summed by one lane in ascending order: np.cumsum bit for bit), F and prev live in LDS: SUMS arrays of
// double[max_len], then F, then prev, 20 bytes a row for one sum and 36 for three.  Lane l takes the candidates l, l + 64, ...
// in ascending index and keeps the first minimum; a xor butterfly over (value, CLASSES * index + class) that prefers the lower
// index on equal values leaves the same pair in every lane.  That pair is the minimum of a total order, so it does not depend
// on how the candidates were dealt: the lowest index among equal minima, as np.argmin gives it.  A workgroup of one wave needs
// no s_barrier (the compiler drops it; __syncthreads is then the LDS fence alone), which is what the many short tracks of a
// real movie want: a step of a track of up to 64 + 2 min_len increments is one pass of the wave.  The whole wave then walks
// prev back from the last increment and writes each stretch's rows straight to global memory.  No atomics, the mapping does
// not depend on the batch: a track's result is bitwise the same alone and in any batch.
//
// mivit_segment_stats and mivit_transport_stats, one launch of stretch_stats_kernel<CENTRED>: one thread per stretch, sums in
// ascending index, no log: bitwise the numpy restatements.  CENTRED takes the stretch's mean increment out first.
// mivit_markov_states, one launch: one thread per particle walks its T uniforms; adds and compares only: bitwise as well.
//
// No contraction into FMA, as in diffusion.hip.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int SEG_THREADS = 64;       // one wave
constexpr int SEG_MAX_LEN = 4096;     // rows of a track: 20 or 36 B a row of LDS, 80 or 144 KiB (ops.SEG_MAX_LEN)
constexpr int STAT_THREADS = 256;
constexpr int MARKOV_THREADS = 64;
constexpr int MARKOV_MAX_K = 8;       // ops.MARKOV_MAX_K

// stretches of one step variance.  cost: C(i, j) of n = j - i increments whose sums are d, and the class of the stretch
struct VarianceModel {
    static constexpr int SUMS = 1, CLASSES = 1;
    static __device__ __forceinline__ void terms(double dy, double dx, double (&t)[SUMS]) { t[0] = dy * dy + dx * dx; }
    static __device__ __forceinline__ double cost(const double (&d)[SUMS], int n, double min_var, double gamma, int &cls) {
        const double tn = 2.0 * (double)n;
        double r = d[0] / tn;
        r = r < min_var ? min_var : r;                                    // np.maximum: a NaN stays
        cls = 0;
        return tn * log(r);
    }
};

// stretches that are diffusive (class 0: the cost above) or directed (class 1: the variance about a constant velocity, plus
// gamma), whichever is lower; a tie is diffusive.  DIRECTED: directed always
template <bool DIRECTED>
struct TransportModel {
    static constexpr int SUMS = 3, CLASSES = 2;
    static __device__ __forceinline__ void terms(double dy, double dx, double (&t)[SUMS]) {
        t[0] = dy * dy + dx * dx;
        t[1] = dy;
        t[2] = dx;
    }
    static __device__ __forceinline__ double cost(const double (&d)[SUMS], int n, double min_var, double gamma, int &cls) {
        const double ss[1] = {d[0]};
        const double c0 = DIRECTED ? 0.0 : VarianceModel::cost(ss, n, min_var, gamma, cls);
        const double tn = 2.0 * (double)n;
        const double m = (d[1] * d[1] + d[2] * d[2]) / (double)n;
        double r = (d[0] - m) / tn;
        r = r < min_var ? min_var : r;                                    // a residual that rounding made negative as well
        const double c1 = tn * log(r) + gamma;
        cls = DIRECTED || c1 < c0 ? 1 : 0;
        return cls ? c1 : c0;
    }
};

template <class M>
constexpr size_t partition_lds_bytes(int rows) { return (size_t)rows * ((M::SUMS + 1) * sizeof(double) + sizeof(int)); }

// seg_class may be null (uniform over the grid): then it is not written
template <class M>
__global__ __launch_bounds__(SEG_THREADS) void partition_kernel(const double *__restrict__ pos, int N,
                                                                const int *__restrict__ offsets, int min_len, double penalty,
                                                                double velocity_penalty, double min_var, int max_len,
                                                                int *__restrict__ seg_start, int *__restrict__ seg_class,
                                                                double *__restrict__ cost) {
    extern __shared__ double seg_lds[];
    double *cs = seg_lds;                                                 // [SUMS][max_len]: cs[s][j] = t_0 + .. + t_{j-1}
    double *F = cs + M::SUMS * max_len;                                   // [max_len]
    int *prev = reinterpret_cast<int *>(F + max_len);                     // [max_len]: CLASSES * i + the class of the stretch (i, j)
    const int k = blockIdx.x, lane = threadIdx.x;
    int a = offsets[k], b = offsets[k + 1];
    a = a < 0 ? 0 : (a > N ? N : a);                                      // never read outside pos, whatever offsets holds
    b = b < a ? a : (b > N ? N : b);
    int L = b - a;
    if (L > max_len) L = max_len;                                         // never write outside LDS (the host checked)
    const int Linc = L - 1;
    if (Linc < 1) {                                                       // uniform over the wave
        if (lane == 0) {
            if (L == 1) {
                seg_start[a] = 1;
                if (seg_class) seg_class[a] = 0;
            }
            cost[k] = NAN;
        }
        return;
    }
    const double *p = pos + (int64_t)a * 2;
    for (int r = lane; r < Linc; r += SEG_THREADS) {
        const double dy = p[2 * (r + 1)] - p[2 * r], dx = p[2 * (r + 1) + 1] - p[2 * r + 1];
        double t[M::SUMS];
        M::terms(dy, dx, t);
#pragma unroll
        for (int s = 0; s < M::SUMS; ++s) cs[s * max_len + r + 1] = t[s];
    }
    __syncthreads();
    if (lane < M::SUMS) {                                                 // the sums side by side
        double *c = cs + lane * max_len;
        double run = 0.0;
        c[0] = 0.0;
        for (int r = 1; r <= Linc; ++r) {
            run = run + c[r];
            c[r] = run;
        }
    }
    __syncthreads();
    const double lg = log((double)Linc);
    const double beta = penalty * lg, gamma = velocity_penalty * lg;
    double fl;
    int pj;                                                               // prev of the last step, or the one stretch's class
    if (Linc < min_len) {                                                 // the recurrence has no step: one stretch
        double d[M::SUMS];
#pragma unroll
        for (int s = 0; s < M::SUMS; ++s) d[s] = cs[s * max_len + Linc];
        fl = (-beta + M::cost(d, Linc, min_var, gamma, pj)) + beta;
    } else {
        if (lane == 0) F[0] = -beta;
        __syncthreads();
        fl = 0.0;
        pj = 0;
        // One wave a CU hides no instruction fetch, and the candidate loop is most of a long track's time: its speed depends
        // on the 4-byte phase at which the loop starts (measured, DESIGN 4w: the one-class loop 40.0 .. 40.6 ms at an odd
        // phase, 41.5 .. 42.4 ms at an even one, 64 tracks of 4096 rows).  The 27 dwords between here and that loop put it at
        // phase 3 of 8 whatever precedes; at most 7 s_nop, once a track.  The two-class loops do not gain by it.
        if (M::CLASSES == 1) asm volatile(".p2align 5");
        for (int j = min_len; j <= Linc; ++j) {
            const int ncand = 1 + (j - 2 * min_len + 1 > 0 ? j - 2 * min_len + 1 : 0);     // i = 0, then min_len .. j - min_len
            double cj[M::SUMS];
#pragma unroll
            for (int s = 0; s < M::SUMS; ++s) cj[s] = cs[s * max_len + j];
            double bv = INFINITY;
            int bi = 0x7fffffff;
            for (int c = lane; c < ncand; c += SEG_THREADS) {
                const int i = c == 0 ? 0 : min_len + c - 1;
                const double fi = F[i];
                double d[M::SUMS];
#pragma unroll
                for (int s = 0; s < M::SUMS; ++s) d[s] = cj[s] - cs[s * max_len + i];
                int cls;
                const double v = (fi + M::cost(d, j - i, min_var, gamma, cls)) + beta;
                if (v < bv) {                                             // ascending i: the first minimum stays
                    bv = v;
                    bi = M::CLASSES * i + cls;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ov < bv || (ov == bv && oi < bi)) {                   // two candidates never share an index
                    bv = ov;
                    bi = oi;
                }
            }
            if (bi >= M::CLASSES * j) bi = 0;                             // only where every candidate was NaN: class 0
            if (lane == 0) {
                F[j] = bv;
                prev[j] = bi;
            }
            fl = bv;
            pj = bi;
            __syncthreads();                                              // one wave: the LDS fence, no s_barrier
        }
    }
    if (lane == 0) cost[k] = fl;
    pj = __builtin_amdgcn_readfirstlane(pj);                              // the same in every lane: the walk is scalar
    int j = Linc;
    while (j > 0) {                                                       // i < j always: at most Linc rounds, L stores in all
        int i = pj / M::CLASSES;
        const int cls = pj % M::CLASSES;
        if (i >= j) i = 0;
        const int hi = j == Linc ? L : j;                                 // the last stretch owns the last row
        for (int r = i + lane; r < hi; r += SEG_THREADS) {
            seg_start[a + r] = r == i ? 1 : 0;
            if (seg_class) seg_class[a + r] = cls;
        }
        // i > 0 was a candidate: min_len <= i <= Linc - min_len, a step of the recurrence, which wrote prev[i]
        if (i > 0) pj = __builtin_amdgcn_readfirstlane(prev[i]);
        j = i;
    }
}

// velocity is written where CENTRED; d_var is D_res where CENTRED, D_mle otherwise
template <bool CENTRED>
__global__ __launch_bounds__(STAT_THREADS) void stretch_stats_kernel(const double *__restrict__ pos, int N,
                                                                     const int *__restrict__ seg_offsets,
                                                                     const int *__restrict__ seg_track_end, int n_seg, double dt,
                                                                     double R, double *__restrict__ velocity,
                                                                     double *__restrict__ d_var, double *__restrict__ d_cve,
                                                                     double *__restrict__ sigma2, int *__restrict__ n_inc) {
    const int s = blockIdx.x * STAT_THREADS + threadIdx.x;
    if (s >= n_seg) return;
    int r0 = seg_offsets[s], r1 = seg_offsets[s + 1];
    const int e = seg_track_end[s] - 1;
    if (r1 > e) r1 = e;                                                   // the bridging increment, unless the track ends
    if (r1 > N - 1) r1 = N - 1;                                           // never read outside pos
    if (r0 < 0) r0 = 0;
    const int n = r1 > r0 ? r1 - r0 : 0;
    double my = NAN, mx = NAN;
    if (CENTRED) {                                                        // pass 1: the mean increment
        double sy = 0.0, sx = 0.0;
        for (int i = 0; i < n; ++i) {
            const double *q = pos + (int64_t)(r0 + i) * 2;
            sy = sy + (q[2] - q[0]);
            sx = sx + (q[3] - q[1]);
        }
        if (n >= 1) {
            my = sy / (double)n;
            mx = sx / (double)n;
        }
    }
    double S2 = 0.0, S11 = 0.0, py = 0.0, px = 0.0;
    for (int i = 0; i < n; ++i) {                                         // the increments, centred where CENTRED
        const double *q = pos + (int64_t)(r0 + i) * 2;
        double dy = q[2] - q[0], dx = q[3] - q[1];
        if (CENTRED) {
            dy = dy - my;
            dx = dx - mx;
        }
        S2 = S2 + (dy * dy + dx * dx);
        if (i > 0) S11 = S11 + (py * dy + px * dx);
        py = dy;
        px = dx;
    }
    double var = NAN, cve = NAN, sg = NAN;
    if (n >= 1) var = S2 / ((4.0 * (double)n) * dt);
    if (n >= 2) {
        const double m1 = 2.0 * (double)(n - 1);
        cve = var + S11 / (m1 * dt);
        sg = (R * S2) / (2.0 * (double)n) + ((2.0 * R - 1.0) * S11) / m1;
    }
    if (CENTRED) {
        velocity[2 * (int64_t)s] = my / dt;
        velocity[2 * (int64_t)s + 1] = mx / dt;
    }
    d_var[s] = var;
    d_cve[s] = cve;
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

// what mivit_segment_tracks and mivit_segment_transport check alike; name is the entry's, for the message
int partition_check(const char *name, const double *pos, int N, const int *offsets, int n_tracks, int max_len, int min_len,
                    double penalty, double min_var, const int *seg_start, const double *cost) {
    MIVIT_CHECK(N >= 0 && n_tracks >= 0, "%s: N = %d, n_tracks = %d: negative size", name, N, n_tracks);
    MIVIT_CHECK(min_len >= 2, "%s: min_len = %d, a stretch needs at least 2 increments", name, min_len);
    MIVIT_CHECK(max_len >= 0 && max_len <= SEG_MAX_LEN,
                "%s: a track of %d rows, the limit is %d (the recurrence's state lives in LDS)", name, max_len, SEG_MAX_LEN);
    MIVIT_CHECK(penalty >= 0.0, "%s: penalty = %g must be >= 0", name, penalty);
    MIVIT_CHECK(min_var > 0.0 && min_var < INFINITY, "%s: min_var = %g must be positive and finite", name, min_var);
    if (n_tracks == 0) return 0;
    MIVIT_CHECK(offsets && cost, "%s: null pointer", name);
    MIVIT_CHECK((pos && seg_start) || N == 0, "%s: null pointer", name);
    return 0;
}

template <class M>
int partition_launch(const double *pos, int N, const int *offsets, int n_tracks, int max_len, int min_len, double penalty,
                     double velocity_penalty, double min_var, int *seg_start, int *seg_class, double *cost, void *stream) {
    const int rows = max_len < 2 ? 2 : max_len;
    const size_t bytes = partition_lds_bytes<M>(rows);
    if (bytes > 48 * 1024)
        MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(partition_kernel<M>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(partition_kernel<M>, dim3((unsigned)n_tracks), dim3(SEG_THREADS), bytes, static_cast<hipStream_t>(stream),
                       pos, N, offsets, min_len, penalty, velocity_penalty, min_var, rows, seg_start, seg_class, cost);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

// what mivit_segment_stats and mivit_transport_stats check alike
int stretch_stats_check(const char *name, const double *pos, int N, int n_seg, double dt, double R, bool outputs) {
    MIVIT_CHECK(N >= 0 && n_seg >= 0, "%s: N = %d, n_seg = %d: negative size", name, N, n_seg);
    MIVIT_CHECK(dt > 0.0 && dt < INFINITY, "%s: dt = %g must be positive and finite", name, dt);
    MIVIT_CHECK(R >= 0.0 && R <= 0.25, "%s: blur coefficient R = %g outside [0, 1/4]", name, R);
    if (n_seg == 0) return 0;
    MIVIT_CHECK(outputs, "%s: null pointer", name);
    MIVIT_CHECK(pos || N == 0, "%s: null pointer", name);
    return 0;
}

template <bool CENTRED>
int stretch_stats_launch(const double *pos, int N, const int *seg_offsets, const int *seg_track_end, int n_seg, double dt,
                         double R, double *velocity, double *d_var, double *d_cve, double *sigma2, int *n_increments,
                         void *stream) {
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(stretch_stats_kernel<CENTRED>, dim3((unsigned)ceil_div(n_seg, STAT_THREADS)), dim3(STAT_THREADS), 0,
                       static_cast<hipStream_t>(stream), pos, N, seg_offsets, seg_track_end, n_seg, dt, R, velocity, d_var, d_cve,
                       sigma2, n_increments);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int mivit_segment_tracks(const double *pos, int N, const int *offsets, int n_tracks, int max_len, int min_len,
                                    double penalty, double min_var, int *seg_start, double *cost, void *stream) {
    if (partition_check("segment_tracks", pos, N, offsets, n_tracks, max_len, min_len, penalty, min_var, seg_start, cost)) return 1;
    if (n_tracks == 0) return 0;
    return partition_launch<VarianceModel>(pos, N, offsets, n_tracks, max_len, min_len, penalty, 0.0, min_var, seg_start, nullptr,
                                           cost, stream);
}

extern "C" int mivit_segment_transport(const double *pos, int N, const int *offsets, int n_tracks, int max_len, int min_len,
                                       double penalty, double velocity_penalty, double min_var, int classes, int *seg_start,
                                       int *seg_class, double *cost, void *stream) {
    MIVIT_CHECK(velocity_penalty >= 0.0, "segment_transport: velocity_penalty = %g must be >= 0", velocity_penalty);
    MIVIT_CHECK(classes >= 0 && classes <= 2, "segment_transport: classes = %d, 0 (both), 1 (directed) or 2 (diffusive)", classes);
    if (partition_check("segment_transport", pos, N, offsets, n_tracks, max_len, min_len, penalty, min_var, seg_start, cost))
        return 1;
    if (n_tracks == 0) return 0;
    MIVIT_CHECK(seg_class || N == 0, "segment_transport: null pointer");
    if (classes == 0)
        return partition_launch<TransportModel<false>>(pos, N, offsets, n_tracks, max_len, min_len, penalty, velocity_penalty,
                                                       min_var, seg_start, seg_class, cost, stream);
    if (classes == 1)
        return partition_launch<TransportModel<true>>(pos, N, offsets, n_tracks, max_len, min_len, penalty, velocity_penalty,
                                                      min_var, seg_start, seg_class, cost, stream);
    return partition_launch<VarianceModel>(pos, N, offsets, n_tracks, max_len, min_len, penalty, velocity_penalty, min_var,
                                           seg_start, seg_class, cost, stream);
}

extern "C" int mivit_segment_stats(const double *pos, int N, const int *seg_offsets, const int *seg_track_end, int n_seg,
                                   double dt, double R, double *d_cve, double *d_mle, double *sigma2, int *n_increments,
                                   void *stream) {
    if (stretch_stats_check("segment_stats", pos, N, n_seg, dt, R,
                            seg_offsets && seg_track_end && d_cve && d_mle && sigma2 && n_increments))
        return 1;
    if (n_seg == 0) return 0;
    return stretch_stats_launch<false>(pos, N, seg_offsets, seg_track_end, n_seg, dt, R, nullptr, d_mle, d_cve, sigma2,
                                       n_increments, stream);
}

extern "C" int mivit_transport_stats(const double *pos, int N, const int *seg_offsets, const int *seg_track_end, int n_seg,
                                     double dt, double R, double *velocity, double *d_res, double *d_cve, double *sigma2,
                                     int *n_increments, void *stream) {
    if (stretch_stats_check("transport_stats", pos, N, n_seg, dt, R,
                            seg_offsets && seg_track_end && velocity && d_res && d_cve && sigma2 && n_increments))
        return 1;
    if (n_seg == 0) return 0;
    return stretch_stats_launch<true>(pos, N, seg_offsets, seg_track_end, n_seg, dt, R, velocity, d_res, d_cve, sigma2,
                                      n_increments, stream);
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
