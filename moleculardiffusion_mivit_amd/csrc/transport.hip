// Run-and-pause transport: the optimal partition of a track into stretches that are each either diffusive (zero-mean
// increments of one variance) or directed (one variance about a constant velocity), and one row of estimates per stretch
// about the stretch's own velocity (no counterpart in the reference; the recurrence is that of csrc/segment.hip, the
// estimators are Vestergaard, Blainey & Flyvbjerg, Phys. Rev. E 89, 022726 (2014) on the centred increments).
// include/mivit_hip.h spells the arithmetic out; helpers/msd.py restates it in numpy.
//
// mivit_segment_transport, one launch: ONE WAVE per track, as seg_tracks_kernel.  Three prefix sums instead of one (of
// dy^2 + dx^2, of dy and of dx; lanes 0, 1 and 2 each sum one sequentially: np.cumsum bit for bit), F and prev in LDS, 36
// bytes a row.  The cost of a candidate stretch is the lower of the diffusive cost C0 (the operations of segment.hip in
// their order) and the directed cost C1 (the velocity profiled out per axis, plus gamma); the class of the winning
// candidate travels through the butterfly in bit 30 of its index and is stored with prev[j].  The butterfly compares (value,
// index): the minimum of a total order, the lowest index among equal minima.  One wave needs no s_barrier.  No atomics, the
// mapping does not depend on the batch: a track's result is bitwise the same alone and in any batch.
//
// mivit_transport_stats, one launch: one thread per stretch, two passes in ascending index, no log: bitwise the numpy
// restatement.
//
// No contraction into FMA, as in segment.hip.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int TR_THREADS = 64;        // one wave
constexpr int TR_MAX_LEN = 4096;      // rows of a track: 36 B a row of LDS, 144 KiB (ops.TRANSPORT_MAX_LEN)
constexpr int TR_STAT_THREADS = 256;
constexpr int TR_IDX = 0x1fffffff;    // prev[j]: the index; bit 30 the class of the stretch that ends at j

__host__ __device__ constexpr size_t tr_lds_bytes(int rows) { return (size_t)rows * (4 * sizeof(double) + sizeof(int)); }

// C(i, j) of n = j - i increments: ss the sum of their squared lengths, sy and sx the sums per axis.  CLASSES 0: the lower of
// the two and its class (a tie is diffusive), 1: directed always, 2: diffusive always.
template <int CLASSES>
__device__ __forceinline__ double tr_cost(double ss, double sy, double sx, int n, double min_var, double gamma, int &cls) {
    const double tn = 2.0 * (double)n;
    double c0 = 0.0, c1 = 0.0;
    if (CLASSES != 1) {
        double r = ss / tn;
        r = r < min_var ? min_var : r;                                    // np.maximum: a NaN stays
        c0 = tn * log(r);
    }
    if (CLASSES != 2) {
        const double m = (sy * sy + sx * sx) / (double)n;
        double r = (ss - m) / tn;
        r = r < min_var ? min_var : r;                                    // a residual that rounding made negative as well
        c1 = tn * log(r) + gamma;
    }
    if (CLASSES == 1) {
        cls = 1;
        return c1;
    }
    if (CLASSES == 2) {
        cls = 0;
        return c0;
    }
    cls = c1 < c0 ? 1 : 0;
    return c1 < c0 ? c1 : c0;
}

template <int CLASSES>
__global__ __launch_bounds__(TR_THREADS) void transport_kernel(const double *__restrict__ pos, int N,
                                                               const int *__restrict__ offsets, int min_len, double penalty,
                                                               double velocity_penalty, double min_var, int max_len,
                                                               int *__restrict__ seg_start, int *__restrict__ seg_class,
                                                               double *__restrict__ cost) {
    extern __shared__ double tr_lds[];
    double *cs2 = tr_lds;                                                 // [max_len]: cs2[j] = q_0 + .. + q_{j-1}
    double *csy = cs2 + max_len;                                          // [max_len]: of dy
    double *csx = csy + max_len;                                          // [max_len]: of dx
    double *F = csx + max_len;                                            // [max_len]
    int *prev = reinterpret_cast<int *>(F + max_len);                     // [max_len]
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
                seg_class[a] = 0;
            }
            cost[k] = NAN;
        }
        return;
    }
    const double *p = pos + (int64_t)a * 2;
    for (int r = lane; r < L; r += TR_THREADS) {
        prev[r] = 0;
        if (r < Linc) {
            const double dy = p[2 * (r + 1)] - p[2 * r], dx = p[2 * (r + 1) + 1] - p[2 * r + 1];
            cs2[r + 1] = dy * dy + dx * dx;
            csy[r + 1] = dy;
            csx[r + 1] = dx;
        }
    }
    __syncthreads();
    if (lane < 3) {                                                       // the three sums side by side
        double *c = lane == 0 ? cs2 : (lane == 1 ? csy : csx);
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
        int cls;
        fl = (-beta + tr_cost<CLASSES>(cs2[Linc], csy[Linc], csx[Linc], Linc, min_var, gamma, cls)) + beta;
        pj = cls << 30;
    } else {
        if (lane == 0) F[0] = -beta;
        __syncthreads();
        fl = 0.0;
        pj = 0;
        for (int j = min_len; j <= Linc; ++j) {
            const int ncand = 1 + (j - 2 * min_len + 1 > 0 ? j - 2 * min_len + 1 : 0);     // i = 0, then min_len .. j - min_len
            const double c2j = cs2[j], cyj = csy[j], cxj = csx[j];
            double bv = INFINITY;
            int bi = 0x7fffffff;
            for (int c = lane; c < ncand; c += TR_THREADS) {
                const int i = c == 0 ? 0 : min_len + c - 1;
                int cls;
                const double v = (F[i] + tr_cost<CLASSES>(c2j - cs2[i], cyj - csy[i], cxj - csx[i], j - i, min_var, gamma, cls)) + beta;
                if (v < bv) {                                             // ascending i: the first minimum stays
                    bv = v;
                    bi = i | (cls << 30);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ov < bv || (ov == bv && (oi & TR_IDX) < (bi & TR_IDX))) {
                    bv = ov;
                    bi = oi;
                }
            }
            if ((bi & TR_IDX) >= j) bi = 0;                               // only where every candidate was NaN: class 0
            if (lane == 0) {
                F[j] = bv;
                prev[j] = bi;
            }
            fl = bv;
            pj = bi;
            __syncthreads();                                              // one wave: the LDS fence, no s_barrier
        }
    }
    if (lane == 0) {
        cost[k] = fl;
        int j = Linc;
        while (j > 0) {                                                   // i < j always: at most Linc rounds, L stores in all
            int i = pj & TR_IDX;
            const int cls = (pj >> 30) & 1;
            if (i >= j) i = 0;
            pj = prev[i];                                                 // as the recurrence left it: rows below j are untouched
            const int hi = j == Linc ? L : j;                             // the last stretch owns the last row
            for (int r = i; r < hi; ++r) prev[r] = (r == i ? (int)0x80000000 : 0) | (cls << 29);
            j = i;
        }
    }
    __syncthreads();
    for (int r = lane; r < L; r += TR_THREADS) {
        const int v = prev[r];
        seg_start[a + r] = v < 0 ? 1 : 0;
        seg_class[a + r] = (v >> 29) & 1;
    }
}

__global__ __launch_bounds__(TR_STAT_THREADS) void transport_stats_kernel(const double *__restrict__ pos, int N,
                                                                          const int *__restrict__ seg_offsets,
                                                                          const int *__restrict__ seg_track_end, int n_seg,
                                                                          double dt, double R, double *__restrict__ velocity,
                                                                          double *__restrict__ d_res, double *__restrict__ d_cve,
                                                                          double *__restrict__ sigma2, int *__restrict__ n_inc) {
    const int s = blockIdx.x * TR_STAT_THREADS + threadIdx.x;
    if (s >= n_seg) return;
    int r0 = seg_offsets[s], r1 = seg_offsets[s + 1];
    const int e = seg_track_end[s] - 1;
    if (r1 > e) r1 = e;                                                   // the bridging increment, unless the track ends
    if (r1 > N - 1) r1 = N - 1;                                           // never read outside pos
    if (r0 < 0) r0 = 0;
    const int n = r1 > r0 ? r1 - r0 : 0;
    double sy = 0.0, sx = 0.0;
    for (int i = 0; i < n; ++i) {                                         // pass 1: the mean increment
        const double *q = pos + (int64_t)(r0 + i) * 2;
        sy = sy + (q[2] - q[0]);
        sx = sx + (q[3] - q[1]);
    }
    double my = NAN, mx = NAN;
    if (n >= 1) {
        my = sy / (double)n;
        mx = sx / (double)n;
    }
    double S2 = 0.0, S11 = 0.0, py = 0.0, px = 0.0;
    for (int i = 0; i < n; ++i) {                                         // pass 2: on the centred increments
        const double *q = pos + (int64_t)(r0 + i) * 2;
        const double ey = (q[2] - q[0]) - my, ex = (q[3] - q[1]) - mx;
        S2 = S2 + (ey * ey + ex * ex);
        if (i > 0) S11 = S11 + (py * ey + px * ex);
        py = ey;
        px = ex;
    }
    double res = NAN, cve = NAN, sg = NAN;
    if (n >= 1) res = S2 / ((4.0 * (double)n) * dt);
    if (n >= 2) {
        const double m1 = 2.0 * (double)(n - 1);
        cve = res + S11 / (m1 * dt);
        sg = (R * S2) / (2.0 * (double)n) + ((2.0 * R - 1.0) * S11) / m1;
    }
    velocity[2 * (int64_t)s] = my / dt;
    velocity[2 * (int64_t)s + 1] = mx / dt;
    d_res[s] = res;
    d_cve[s] = cve;
    sigma2[s] = sg;
    n_inc[s] = n;
}

template <int CLASSES>
int transport_launch(const double *pos, int N, const int *offsets, int n_tracks, int rows, int min_len, double penalty,
                     double velocity_penalty, double min_var, int *seg_start, int *seg_class, double *cost, void *stream) {
    const size_t bytes = tr_lds_bytes(rows);
    if (bytes > 48 * 1024)
        MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(transport_kernel<CLASSES>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(transport_kernel<CLASSES>, dim3((unsigned)n_tracks), dim3(TR_THREADS), bytes,
                       static_cast<hipStream_t>(stream), pos, N, offsets, min_len, penalty, velocity_penalty, min_var, rows,
                       seg_start, seg_class, cost);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int mivit_segment_transport(const double *pos, int N, const int *offsets, int n_tracks, int max_len, int min_len,
                                       double penalty, double velocity_penalty, double min_var, int classes, int *seg_start,
                                       int *seg_class, double *cost, void *stream) {
    MIVIT_CHECK(N >= 0 && n_tracks >= 0, "segment_transport: N = %d, n_tracks = %d: negative size", N, n_tracks);
    MIVIT_CHECK(min_len >= 2, "segment_transport: min_len = %d, a stretch needs at least 2 increments", min_len);
    MIVIT_CHECK(max_len >= 0 && max_len <= TR_MAX_LEN,
                "segment_transport: a track of %d rows, the limit is %d (the recurrence's state lives in LDS)", max_len, TR_MAX_LEN);
    MIVIT_CHECK(penalty >= 0.0, "segment_transport: penalty = %g must be >= 0", penalty);
    MIVIT_CHECK(velocity_penalty >= 0.0, "segment_transport: velocity_penalty = %g must be >= 0", velocity_penalty);
    MIVIT_CHECK(min_var > 0.0 && min_var < INFINITY, "segment_transport: min_var = %g must be positive and finite", min_var);
    MIVIT_CHECK(classes >= 0 && classes <= 2, "segment_transport: classes = %d, 0 (both), 1 (directed) or 2 (diffusive)", classes);
    if (n_tracks == 0) return 0;
    MIVIT_CHECK(offsets && cost, "segment_transport: null pointer");
    MIVIT_CHECK((pos && seg_start && seg_class) || N == 0, "segment_transport: null pointer");
    const int rows = max_len < 2 ? 2 : max_len;
    if (classes == 0)
        return transport_launch<0>(pos, N, offsets, n_tracks, rows, min_len, penalty, velocity_penalty, min_var, seg_start,
                                   seg_class, cost, stream);
    if (classes == 1)
        return transport_launch<1>(pos, N, offsets, n_tracks, rows, min_len, penalty, velocity_penalty, min_var, seg_start,
                                   seg_class, cost, stream);
    return transport_launch<2>(pos, N, offsets, n_tracks, rows, min_len, penalty, velocity_penalty, min_var, seg_start,
                               seg_class, cost, stream);
}

extern "C" int mivit_transport_stats(const double *pos, int N, const int *seg_offsets, const int *seg_track_end, int n_seg,
                                     double dt, double R, double *velocity, double *d_res, double *d_cve, double *sigma2,
                                     int *n_increments, void *stream) {
    MIVIT_CHECK(N >= 0 && n_seg >= 0, "transport_stats: N = %d, n_seg = %d: negative size", N, n_seg);
    MIVIT_CHECK(dt > 0.0 && dt < INFINITY, "transport_stats: dt = %g must be positive and finite", dt);
    MIVIT_CHECK(R >= 0.0 && R <= 0.25, "transport_stats: blur coefficient R = %g outside [0, 1/4]", R);
    if (n_seg == 0) return 0;
    MIVIT_CHECK(seg_offsets && seg_track_end && velocity && d_res && d_cve && sigma2 && n_increments,
                "transport_stats: null pointer");
    MIVIT_CHECK(pos || N == 0, "transport_stats: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(transport_stats_kernel, dim3((unsigned)ceil_div(n_seg, TR_STAT_THREADS)), dim3(TR_STAT_THREADS), 0,
                       static_cast<hipStream_t>(stream), pos, N, seg_offsets, seg_track_end, n_seg, dt, R, velocity, d_res, d_cve,
                       sigma2, n_increments);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
