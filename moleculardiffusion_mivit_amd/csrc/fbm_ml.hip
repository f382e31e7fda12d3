// Per-track maximum-likelihood anomalous exponent and generalised diffusion coefficient with error bars, from rows that each
// carry their own variance (no counterpart in the reference).  The model is the exact Gaussian likelihood of a track's
// increments under fractional Brownian motion averaged over an exposure, localisation noise of known, row-dependent variance
// and missing frames: the DENSE covariance of include/mivit_hip.h (mivit_track_fbm_loglik), which at alpha = 1 is the
// tridiagonal one of csrc/likelihood.hip.  helpers/msd._fbm_ml_numpy restates the search in numpy with LAPACK's Cholesky.
//
// ONE WORKGROUP PER (RANGE, CANDIDATE), 192 threads.  The workgroup compacts the usable rows of its range into LDS (ballots,
// one pass), builds the table S(0 .. span) of the structure function for its alpha, and per axis builds the covariance as a
// packed lower triangle in LDS with the increments as one more row below it, so that the left-looking factorisation
// leaves L^-1 d in that row: thread i owns row i and forms its own dot products in ascending k and the running value of its
// own pivot, which it publishes in the diagonal's place one column before the others need it, so a column costs one barrier
// and no value crosses threads through anything but LDS.  The thread of the increments' row takes the determinant as an exactly
// rescaled product (frexp) and the quadratic form in column order.  The two axes have their own
// variances and therefore their own factorisation, one after the other in the same triangle.  The usable-row rule, the
// product, the closing of the cost and the stencil's information matrix are those of track_ml.h.
//
// The search runs without the host: per round one launch of n x 64 workgroups writes the 64 costs of every range into the
// caller's workspace and a one-thread-per-range kernel takes the arg-min (lowest index on a tie) and writes the next
// bracket; 20 rounds, then n x 9 workgroups for the stencil of the error bars and one thread per range for the outputs.
// fp64 without contraction, no atomics, no scratch; a range's work does not depend on where it sits in a batch.
#pragma clang fp contract(off)

#include "track_ml.h"

namespace {

constexpr int FM_THREADS = 192;                                           // >= FM_MAX_ROWS: rows 0 .. m - 1 and the increments' row m
constexpr int FM_MAX_ROWS = 129;                                          // usable rows of a range (ops.FBM_ML_MAX_ROWS)
constexpr int FM_MAX_INC = FM_MAX_ROWS - 1;
constexpr int FM_MAX_SPAN = 1199;                                         // last usable frame - first (ops.FBM_ML_MAX_SPAN)
constexpr int FM_TRI = (FM_MAX_INC + 1) * (FM_MAX_INC + 2) / 2;           // packed rows 0 .. FM_MAX_INC
constexpr int FM_LDS_DOUBLES = FM_TRI + (FM_MAX_SPAN + 1) + 2 * FM_MAX_INC + 2 * FM_MAX_ROWS;
constexpr int FM_LDS_BYTES = FM_LDS_DOUBLES * 8 + (FM_MAX_ROWS + 3) * 4;  // + frames and the three wave counts: 81 320 B
constexpr int FM_CAND = 64, FM_ROUNDS = 20, FM_TERMS = 30;
constexpr double FM_ALPHA_MIN = 0.05, FM_ALPHA_MAX = 1.95;               // helpers/generation.ALPHA_MIN, ALPHA_MAX
constexpr double FM_U_LO = -12.0, FM_U_HI = 4.0;                          // the first bracket of log2(D / D_ref)
// the workspace of a range, in doubles: 64 costs (the stencil's 9 over the first of them), the bracket, the two flags, the
// best candidate, and what the last kernel needs of the range
constexpr int FM_WS = 80, FM_WS_ALO = 64, FM_WS_AHI = 65, FM_WS_ULO = 66, FM_WS_UHI = 67, FM_WS_ALL_LO = 68, FM_WS_ALL_HI = 69,
              FM_WS_ALPHA = 70, FM_WS_U = 71, FM_WS_NINC = 72, FM_WS_STATUS = 73, FM_WS_D = 74;

enum { FM_LOGLIK = 0, FM_ROUND = 1, FM_STENCIL = 2 };

struct FmIn {
    const double *pos, *var;
    const int *frames;
    const unsigned char *use;
    const int *offsets;
    int N;
    double dt, E;
};

// the structure function of fractional Brownian motion averaged over the exposure E, at a lag of t frames
__device__ __forceinline__ double fm_structure(double alpha, int t, double E) {
    const double tau = (double)t;
    if (E == 0.0) return t == 0 ? 0.0 : pow(tau, alpha);
    const double a12 = (alpha + 1.0) * (alpha + 2.0);
    if (t == 0) return (2.0 * pow(E, alpha)) / a12;
    if (E > 0.5 * tau) {                                                  // tau = 1 and E > 1/2: the closed form
        const double p = alpha + 2.0;
        return ((pow(tau + E, p) + pow(fabs(tau - E), p)) - 2.0 * pow(tau, p)) / ((E * E) * a12);
    }
    const double x = E / tau, x2 = x * x;
    double term = 1.0, sum = 1.0;
#pragma unroll 1
    for (int m = 1; m <= FM_TERMS; ++m) {
        const double tm = (double)(2 * m);
        term = (term * (((alpha - tm + 2.0) * (alpha - tm + 1.0)) / ((tm + 1.0) * (tm + 2.0)))) * x2;
        sum = sum + term;
    }
    return pow(tau, alpha) * sum;
}

// The usable rows of range k into LDS; every thread returns their number (above FM_MAX_ROWS the LDS holds the first
// FM_MAX_ROWS of them).  Xy, Xx receive the positions.
__device__ __forceinline__ int fm_compact(const FmIn &in, int k, double *Xy, double *Xx, double *vy, double *vx, int *fr, int *wcnt) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    TmRows R;
    R.pos = in.pos, R.var = in.var, R.frames = in.frames, R.use = in.use;
    tm_clamp_range(in.offsets, k, in.N, R.a, R.b);
    int base = 0;
    for (int r0 = R.a; r0 < R.b; r0 += FM_THREADS) {                      // r0 <= N - 1: r0 + tid cannot overflow for N <= 2^31 - 192
        const int r = r0 + tid;
        TmRow row{};                                                      // not usable beyond the range's end
        if (r < R.b) row = tm_row(R, r);
        const bool ok = row.ok;
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < FM_THREADS / 64; ++w) {
            const int c = wcnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        const int idx = base + before + __popcll(bal & ((1ull << lane) - 1ull));
        if (ok && idx < FM_MAX_ROWS) Xy[idx] = row.y, Xx[idx] = row.x, vy[idx] = row.vy, vx[idx] = row.vx, fr[idx] = row.f;
        base += total;
        __syncthreads();
    }
    return base;
}

// -2 log L of one axis: the triangle of this axis' covariance with the increments d below it, factorised in place.  Returns
// in thread m (the increments' row) the sum log det C + d^T C^-1 d through (det, Q); bad where a pivot is not positive.
__device__ __forceinline__ void fm_axis(double *Lp, const double *tab, const double *d, const double *v, const int *fr, int m, double Ddt,
                        double &Q, TmProd &det, bool &bad) {
    const int i = threadIdx.x;
    double *ri = Lp + (i * (i + 1)) / 2;                                  // used where i <= m only
    if (i < m) {
        const int fi = fr[i], fi1 = fr[i + 1];
        for (int j = 0; j <= i; ++j) {
            const int fj = fr[j], fj1 = fr[j + 1];
            const double q = ((tab[abs(fi1 - fj)] + tab[abs(fi - fj1)]) - tab[abs(fi1 - fj1)]) - tab[abs(fi - fj)];
            double c = Ddt * q;
            if (j == i) c = (c + v[i]) + v[i + 1];
            if (j == i - 1) c = c - v[i];
            ri[j] = c;
        }
    } else if (i == m) {
        for (int j = 0; j < m; ++j) ri[j] = d[j];
    }
    __syncthreads();
    // The pivot of row i is a running value of its owner, p_i = C_ii - sum_{k<j} L_ik L_ik, one term a column in ascending k;
    // it is complete after column i - 1 and is published then in the diagonal's place, where column i finds it.
    double pi = i < m ? ri[i] : 0.0;
#pragma unroll 1
    for (int j = 0; j < m; ++j) {
        if (i > j && i <= m) {
            const double *rj = Lp + (j * (j + 1)) / 2;
            const double p = rj[j];
            double s = ri[j];
            for (int k = 0; k < j; ++k) s = s - ri[k] * rj[k];
            s = s / sqrt(p);
            ri[j] = s;
            if (i == m) {
                if (!(p > 0.0)) bad = true;                               // not positive definite (or NaN): the candidate is rejected
                Q = Q + s * s;
                det.mul(p);
            } else {
                pi = pi - s * s;
                if (i == j + 1) ri[i] = pi;
            }
        }
        __syncthreads();
    }
}

// What a workgroup needs of its range: the compacted rows in LDS, the counts and D_ref.  status: 0, 1 or 5.
struct FmRange {
    int m, n_inc, status;
    double D_ref;
};

template <int MODE>
__global__ __launch_bounds__(FM_THREADS) void fm_cost_kernel(FmIn in, const double *__restrict__ alpha_in,
                                                             const double *__restrict__ D_in, int round, double *__restrict__ ws,
                                                             double *__restrict__ loglik, int *__restrict__ n_increments,
                                                             int *__restrict__ status) {
    extern __shared__ double fm_lds[];
    double *Lp = fm_lds, *tab = Lp + FM_TRI, *dy = tab + (FM_MAX_SPAN + 1), *dx = dy + FM_MAX_INC, *vy = dx + FM_MAX_INC,
           *vx = vy + FM_MAX_ROWS;
    int *fr = reinterpret_cast<int *>(vx + FM_MAX_ROWS), *wcnt = fr + FM_MAX_ROWS;
    const int tid = threadIdx.x;
    const int per = MODE == FM_ROUND ? FM_CAND : (MODE == FM_STENCIL ? 9 : 1);
    const int k = blockIdx.x / per, c = blockIdx.x % per;
    double *w = ws ? ws + (int64_t)k * FM_WS : nullptr;

    const int rows = fm_compact(in, k, Lp, Lp + FM_MAX_ROWS, vy, vx, fr, wcnt);      // the positions where the triangle will be
    const int n_inc = rows > 0 ? rows - 1 : 0;
    int st = rows > FM_MAX_ROWS ? 5 : 0;
    const int m = st ? 0 : n_inc;
    // the span of the usable frames, D_ref: the same loop in every thread (LDS broadcasts)
    int fmin = 0, fmax = 0;
    for (int r = 0; r <= m && rows > 0; ++r) {
        const int f = fr[r];
        fmin = r == 0 || f < fmin ? f : fmin;
        fmax = r == 0 || f > fmax ? f : fmax;
    }
    if ((int64_t)fmax - (int64_t)fmin > FM_MAX_SPAN) st = 5;
    if (st == 0 && n_inc < (MODE == FM_LOGLIK ? 1 : 3)) st = 1;
    double alpha = 0.0, D = 0.0;
    if (MODE == FM_LOGLIK) {
        alpha = alpha_in[k], D = D_in[k];
        if (st == 0 && !(alpha > 0.0 && alpha < 2.0 && D >= 0.0 && D < INFINITY)) st = 6;
    }
    if (st) {                                                             // the same in every thread
        if (tid == 0) {
            if (MODE == FM_LOGLIK) loglik[k] = NAN, n_increments[k] = n_inc, status[k] = st;
            if (MODE == FM_ROUND) w[c] = INFINITY;
            if (MODE == FM_STENCIL) {
                w[c] = INFINITY;
                if (c == 4) w[FM_WS_NINC] = (double)n_inc, w[FM_WS_STATUS] = (double)st, w[FM_WS_D] = NAN;
            }
        }
        return;
    }
    const int span = fmax - fmin;
    if (tid < m) {
        dy[tid] = Lp[tid + 1] - Lp[tid];
        dx[tid] = Lp[FM_MAX_ROWS + tid + 1] - Lp[FM_MAX_ROWS + tid];
    }
    __syncthreads();
    if (MODE != FM_LOGLIK) {
        double S = 0.0;
        for (int r = 0; r < m; ++r) S = S + (dy[r] * dy[r] + dx[r] * dx[r]);
        const double D_ref = tm_d_ref(S, in.dt, (int64_t)fr[m] - (int64_t)fr[0]);
        if (MODE == FM_ROUND) {
            const double alo = round ? w[FM_WS_ALO] : FM_ALPHA_MIN, ahi = round ? w[FM_WS_AHI] : FM_ALPHA_MAX;
            const double ulo = round ? w[FM_WS_ULO] : FM_U_LO, uhi = round ? w[FM_WS_UHI] : FM_U_HI;
            alpha = alo + (double)(c >> 3) * ((ahi - alo) / 7.0);
            D = D_ref * exp2(ulo + (double)(c & 7) * ((uhi - ulo) / 7.0));
        } else {
            const double Db = w[FM_WS_ALL_LO] != 0.0 ? 0.0 : D_ref * exp2(w[FM_WS_U]);
            const int ia = c / 3 - 1, id = c % 3 - 1;
            alpha = w[FM_WS_ALPHA] + (double)ia * TM_H;
            D = id > 0 ? Db * TM_EXP_H : (id < 0 ? Db * TM_EXP_MH : Db);
            if (c == 4 && tid == 0) w[FM_WS_NINC] = (double)n_inc, w[FM_WS_STATUS] = 0.0, w[FM_WS_D] = Db;
        }
    }
    for (int t = tid; t <= span; t += FM_THREADS) tab[t] = fm_structure(alpha, t, in.E);
    __syncthreads();                                                      // also: the positions in Lp are no longer needed

    const double Ddt = D * in.dt;
    double Q = 0.0;
    TmProd det;
    bool bad = false;
    fm_axis(Lp, tab, dy, vy, fr, m, Ddt, Q, det, bad);
    fm_axis(Lp, tab, dx, vx, fr, m, Ddt, Q, det, bad);
    if (tid == m) {
        const double cost = tm_finish_cost(det, Q, m, bad);
        if (MODE == FM_LOGLIK)
            loglik[k] = -0.5 * cost, n_increments[k] = n_inc, status[k] = 0;
        else
            w[c] = cost;
    }
}

// between two rounds: the arg-min of the 64 costs of a range (lowest index on a tie) and the next bracket, best +- 2 cells
__global__ void fm_next_kernel(int n, int round, double *__restrict__ ws) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double *w = ws + (int64_t)k * FM_WS;
    const double alo = round ? w[FM_WS_ALO] : FM_ALPHA_MIN, ahi = round ? w[FM_WS_AHI] : FM_ALPHA_MAX;
    const double ulo = round ? w[FM_WS_ULO] : FM_U_LO, uhi = round ? w[FM_WS_UHI] : FM_U_HI;
    int best = 0;
    double cb = w[0];
#pragma unroll 1
    for (int c = 1; c < FM_CAND; ++c) {
        const double cc = w[c];
        if (cc < cb) cb = cc, best = c;
    }
    const int i = best >> 3, j = best & 7;
    const double sa = (ahi - alo) / 7.0, su = (uhi - ulo) / 7.0;
    const double ab = alo + (double)i * sa, ub = ulo + (double)j * su;
    const double nalo = ab - 2.0 * sa, nahi = ab + 2.0 * sa;
    w[FM_WS_ALO] = nalo < FM_ALPHA_MIN ? FM_ALPHA_MIN : nalo;
    w[FM_WS_AHI] = nahi > FM_ALPHA_MAX ? FM_ALPHA_MAX : nahi;
    w[FM_WS_ULO] = ub - 2.0 * su;
    w[FM_WS_UHI] = ub + 2.0 * su;
    const bool all_lo = (round ? w[FM_WS_ALL_LO] != 0.0 : true) && j == 0;
    const bool all_hi = (round ? w[FM_WS_ALL_HI] != 0.0 : true) && j == 7;
    w[FM_WS_ALL_LO] = all_lo ? 1.0 : 0.0;
    w[FM_WS_ALL_HI] = all_hi ? 1.0 : 0.0;
    w[FM_WS_ALPHA] = ab;
    w[FM_WS_U] = ub;
}

// after the stencil: the outputs of a range
__global__ void fm_finish_kernel(int n, const double *__restrict__ ws, double *__restrict__ alpha, double *__restrict__ alpha_std,
                                 double *__restrict__ D, double *__restrict__ D_std, double *__restrict__ corr,
                                 double *__restrict__ loglik, int *__restrict__ n_increments, int *__restrict__ status) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double *w = ws + (int64_t)k * FM_WS;
    int st = (int)w[FM_WS_STATUS];
    double a = NAN, as = NAN, Dk = NAN, Ds = NAN, co = NAN, ll = NAN;
    if (st == 0) {
        st = w[FM_WS_ALL_LO] != 0.0 ? 2 : (w[FM_WS_ALL_HI] != 0.0 ? 3 : 0);
        const double c0 = w[4];
        ll = -0.5 * c0;
        Dk = w[FM_WS_D];
        if (st != 2) {
            a = w[FM_WS_ALPHA];
            const TmHess2 H(w);                                           // u = alpha, v = ln D: the stencil's costs are w[0 .. 8]
            const bool pd = H.pd();
            if (a - TM_H >= FM_ALPHA_MIN && a + TM_H <= FM_ALPHA_MAX && pd) {
                as = sqrt(H.vv / H.det);
                Ds = Dk * sqrt(H.uu / H.det);
                co = -H.uv / sqrt(H.uu * H.vv);
            } else if (st == 0) {
                st = 4;
            }
        }
    }
    alpha[k] = a, alpha_std[k] = as, D[k] = Dk, D_std[k] = Ds, corr[k] = co, loglik[k] = ll;
    n_increments[k] = (int)w[FM_WS_NINC], status[k] = st;
}

template <int MODE>
int fm_launch_cost(const FmIn &in, const double *alpha, const double *D, int n, int round, double *ws, double *loglik,
                   int *n_increments, int *status, hipStream_t s) {
    auto kern = fm_cost_kernel<MODE>;
    MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, FM_LDS_BYTES));
    const int per = MODE == FM_ROUND ? FM_CAND : (MODE == FM_STENCIL ? 9 : 1);
    hipLaunchKernelGGL(kern, dim3((unsigned)n * (unsigned)per), dim3(FM_THREADS), FM_LDS_BYTES, s, in, alpha, D, round, ws, loglik,
                       n_increments, status);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

int fm_check(const char *name, const double *pos, int N, const int *offsets, int n, double dt, double exposure) {
    if (int rc = tm_check_rows(name, pos, N, offsets, n, dt)) return rc;
    MIVIT_CHECK(N <= 2147483647 - FM_THREADS, "%s: N = %d rows, at most %d", name, N, 2147483647 - FM_THREADS);
    MIVIT_CHECK(n <= (1 << 24), "%s: n = %d ranges, at most %d in one call", name, n, 1 << 24);
    MIVIT_CHECK(exposure >= 0.0 && exposure <= 1.0, "%s: exposure = %g outside [0, 1]", name, exposure);
    return 0;
}

}  // namespace

extern "C" int mivit_track_fbm_loglik(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                                      const int *offsets, int n, double dt, double exposure, const double *alpha, const double *D,
                                      double *loglik, int *n_increments, int *status, void *stream) {
    if (int rc = fm_check("track_fbm_loglik", pos, N, offsets, n, dt, exposure)) return rc;
    if (n == 0) return 0;
    MIVIT_CHECK(alpha && D && loglik && n_increments && status, "track_fbm_loglik: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    const FmIn in{pos, var, frames, use, offsets, N, dt, exposure};
    return fm_launch_cost<FM_LOGLIK>(in, alpha, D, n, 0, nullptr, loglik, n_increments, status, static_cast<hipStream_t>(stream));
}

extern "C" int mivit_track_fbm_ml(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                                  const int *offsets, int n, double dt, double exposure, double *alpha, double *alpha_std, double *D,
                                  double *D_std, double *corr, double *loglik, int *n_increments, int *status, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    if (int rc = fm_check("track_fbm_ml", pos, N, offsets, n, dt, exposure)) return rc;
    if (n == 0) return 0;
    MIVIT_CHECK(alpha && alpha_std && D && D_std && corr && loglik && n_increments && status, "track_fbm_ml: null pointer");
    MIVIT_CHECK(workspace && reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "track_fbm_ml: the workspace is null or not 8-byte aligned");
    MIVIT_CHECK(workspace_bytes >= (size_t)n * FM_WS * sizeof(double), "track_fbm_ml: workspace of %zu bytes, %zu needed (640 a range)",
                workspace_bytes, (size_t)n * FM_WS * sizeof(double));
    prof_set_tag(MIVIT_PROF_OP);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FmIn in{pos, var, frames, use, offsets, N, dt, exposure};
    double *ws = static_cast<double *>(workspace);
    const unsigned blocks = ((unsigned)n + 127u) / 128u;
    for (int round = 0; round < FM_ROUNDS; ++round) {
        if (int rc = fm_launch_cost<FM_ROUND>(in, nullptr, nullptr, n, round, ws, nullptr, nullptr, nullptr, s)) return rc;
        hipLaunchKernelGGL(fm_next_kernel, dim3(blocks), dim3(128), 0, s, n, round, ws);
        MIVIT_LAUNCH_CHECK();
    }
    if (int rc = fm_launch_cost<FM_STENCIL>(in, nullptr, nullptr, n, 0, ws, nullptr, nullptr, nullptr, s)) return rc;
    hipLaunchKernelGGL(fm_finish_kernel, dim3(blocks), dim3(128), 0, s, n, static_cast<const double *>(ws), alpha, alpha_std, D, D_std,
                       corr, loglik, n_increments, status);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
