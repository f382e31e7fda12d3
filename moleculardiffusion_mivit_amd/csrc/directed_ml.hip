// Per-track maximum-likelihood velocity and diffusion coefficient of directed motion with error bars, and the exact
// log-likelihood of directed motion at given parameters, from row positions that each carry their own variance (no
// counterpart in the reference).  The model is that of likelihood.hip with a mean: the increments of a track are Gaussian
// with the tridiagonal covariance of mivit_track_diffusion_ml (localisation noise of known, row-dependent variance, motion
// blur, missing frames) about u g dt, u the velocity of the axis.  The velocity enters linearly and is profiled out in closed
// form inside the same LDL^T recurrence: a second recurrence on the mean's regressor with the same multiplier and the same
// pivot, and three sums per axis.  include/mivit_hip.h spells the arithmetic out; helpers/msd._directed_ml_numpy restates it.
//
// ONE WAVE PER RANGE (a workgroup of 64 threads), lane j = candidate j of the fixed grid search over log2 D of
// likelihood.hip.  Every lane walks the same rows, so the row index, the usability test and the loop are wave-uniform and
// only D differs between lanes.  Per axis the last pivot's reciprocal, the two residuals and the three sums, and the running
// determinant live in registers: no LDS, no scratch, no atomics, no barrier, and a range has no maximum length.  The rows
// are read again from global memory in each of the 9 passes (one for the row count and the unweighted velocity, one for
// D_ref, six rounds of the search, one for the three points of the curvature); a range is a few KiB and stays in cache.
//
// The recurrence runs on the increments LESS THE UNWEIGHTED VELOCITY'S SHARE, d - u0 g dt with u0 = (last usable position -
// first) / (G dt): the profile is invariant under that shift (u = u0 + B / C), and with it the three sums stay of the size of
// the noise however fast the track is, so A - B B / C cancels nothing and a velocity added to a track moves D by rounding alone.
// For the same reason the reference scale D_ref is taken from these residuals, not from sum d^2.
//
// The determinant is a PRODUCT rescaled exactly by frexp: no log in the loop.  The arg-min goes through xor shuffles (least
// cost, lowest lane on a tie).  The work of a range does not depend on where it sits in a batch: its outputs are bitwise the
// same alone, anywhere in a batch and in every launch.  The rows, the product, the closing of the cost, the arg-min and the
// curvature are those of track_ml.h.
//
// No contraction into FMA.
#pragma clang fp contract(off)

#include "track_ml.h"

namespace {

constexpr int DM_THREADS = TM_WAVE;                                       // one wave = the candidates of a round
constexpr int DM_ROUNDS = 6;
constexpr double DM_U_LO = -20.0, DM_U_HI = 4.0;                          // the first bracket of log2(D / D_ref)

struct DmFit {
    double cost, uy, ux, Cy, Cx;                                          // -2 log L, the profiled velocity, C per axis
    int cnt;                                                              // usable rows
};

// pass 0: the usable rows, the summed gaps and the unweighted velocity (last usable position - first) / (G dt)
struct DmStart {
    int cnt;
    int64_t G;
    double uy, ux;
};

__device__ __forceinline__ DmStart dm_start(const TmRows &R, double dt) {
    double fy = 0.0, fx = 0.0, ly = 0.0, lx = 0.0;
    int64_t G = 0;
    int pf = 0, cnt = 0;
    for (int r = R.a; r < R.b; ++r) {
        const TmRow w = tm_row(R, r);
        if (!w.ok) continue;
        if (cnt == 0)
            fy = w.y, fx = w.x;
        else
            G += w.f - pf;
        ly = w.y, lx = w.x, pf = w.f;
        ++cnt;
    }
    const double T = (double)G * dt;
    return DmStart{cnt, G, (ly - fy) / T, (lx - fx) / T};
}

// the reference scale: sum (d - u0 m)^2 (both axes) / (4 dt G)
__device__ __forceinline__ double dm_d_ref(const TmRows &R, double dt, const DmStart &s) {
    double S = 0.0, py = 0.0, px = 0.0;
    int pf = 0, cnt = 0;
    for (int r = R.a; r < R.b; ++r) {
        const TmRow w = tm_row(R, r);
        if (!w.ok) continue;
        if (cnt > 0) {
            const double m = (double)(w.f - pf) * dt;
            const double dy = (w.y - py) - s.uy * m, dx = (w.x - px) - s.ux * m;
            S = S + (dy * dy + dx * dx);
        }
        py = w.y, px = w.x, pf = w.f;
        ++cnt;
    }
    return tm_d_ref(S, dt, s.G);
}

// one axis of one increment: the pivot e of ml_axis, the residuals z of the increment and w of the regressor under the same
// multiplier, the three sums and the determinant
__device__ __forceinline__ void dm_axis(bool first, double base, double cR, double pv, double v, double d, double m, double &rinv,
                                        double &z, double &w, double &A, double &B, double &C, TmProd &det, bool &bad) {
    const double a = (base + pv) + v;
    double e;
    if (first) {
        e = a;
        z = d;
        w = m;
    } else {
        const double b = cR - pv;                                         // pv: the variance of the row both increments share
        const double l = b * rinv;
        e = a - l * b;
        z = d - l * z;
        w = m - l * w;
    }
    if (!(e > 0.0)) bad = true;                                           // not positive definite (or NaN): the candidate is rejected
    rinv = 1.0 / e;
    A = A + (z * z) * rinv;
    B = B + (z * w) * rinv;
    C = C + (w * w) * rinv;
    det.mul(e);
}

// -2 log L of the range at D about the velocity (gy, gx) where `given`, else with the velocity profiled; the recurrence runs
// on d - (gy, gx) m either way and the fit's velocity is (gy, gx) + B / C.  +inf for a rejected candidate (a pivot or a C that
// is not positive, a C that is not finite) and for a cost that is not a number
__device__ __forceinline__ DmFit dm_cost(const TmRows &R, double D, double dt, double Rb, bool given, double gy, double gx) {
    const double c1 = (2.0 * D) * dt, cR = Rb * c1, tR = 2.0 * Rb;
    double py = 0.0, px = 0.0, pvy = 0.0, pvx = 0.0;
    double ry = 0.0, rx = 0.0, zy = 0.0, zx = 0.0, wy = 0.0, wx = 0.0;
    double Ay = 0.0, By = 0.0, Cy = 0.0, Ax = 0.0, Bx = 0.0, Cx = 0.0;
    TmProd det;
    int pf = 0, cnt = 0;
    bool bad = false;
    for (int r = R.a; r < R.b; ++r) {
        const TmRow w = tm_row(R, r);
        if (!w.ok) continue;                                              // wave-uniform
        if (cnt > 0) {
            const double g = (double)(w.f - pf);
            const double base = c1 * (g - tR);
            const double m = g * dt;
            dm_axis(cnt == 1, base, cR, pvy, w.vy, (w.y - py) - gy * m, m, ry, zy, wy, Ay, By, Cy, det, bad);
            dm_axis(cnt == 1, base, cR, pvx, w.vx, (w.x - px) - gx * m, m, rx, zx, wx, Ax, Bx, Cx, det, bad);
        }
        py = w.y, px = w.x, pvy = w.vy, pvx = w.vx, pf = w.f;
        ++cnt;
    }
    if (!(Cy > 0.0 && Cy < INFINITY && Cx > 0.0 && Cx < INFINITY)) bad = true;
    DmFit fit;
    const double Q = given ? Ay + Ax : (Ay - (By * By) / Cy) + (Ax - (Bx * Bx) / Cx);
    fit.cost = tm_finish_cost(det, Q, cnt - 1, bad);
    fit.uy = gy + By / Cy, fit.ux = gx + Bx / Cx;
    fit.Cy = Cy, fit.Cx = Cx, fit.cnt = cnt;
    return fit;
}

__global__ __launch_bounds__(DM_THREADS) void dm_kernel(const double *__restrict__ pos, const double *__restrict__ var,
                                                        const int *__restrict__ frames, const unsigned char *__restrict__ use,
                                                        int N, const int *__restrict__ offsets, double dt, double Rb,
                                                        double *__restrict__ D_out, double *__restrict__ D_std,
                                                        double *__restrict__ v_out, double *__restrict__ v_std,
                                                        double *__restrict__ loglik, int *__restrict__ n_increments,
                                                        int *__restrict__ status) {
    const int k = blockIdx.x, lane = threadIdx.x;
    TmRows R;
    R.pos = pos, R.var = var, R.frames = frames, R.use = use;
    tm_clamp_range(offsets, k, N, R.a, R.b);

    // pass 0: the usable rows and the unweighted velocity; the same in every lane
    const DmStart s0 = dm_start(R, dt);
    const int n_inc = s0.cnt > 0 ? s0.cnt - 1 : 0;
    if (n_inc < 2) {                                                      // wave-uniform
        if (lane == 0) {
            D_out[k] = NAN, D_std[k] = NAN, loglik[k] = NAN;
            v_out[2 * (int64_t)k] = NAN, v_out[2 * (int64_t)k + 1] = NAN;
            v_std[2 * (int64_t)k] = NAN, v_std[2 * (int64_t)k + 1] = NAN;
            n_increments[k] = n_inc, status[k] = 1;
        }
        return;
    }
    // pass 1: D_ref from the residuals about the unweighted velocity
    const double D_ref = dm_d_ref(R, dt, s0);

    // the search of likelihood.hip: 64 candidates over the bracket, the bracket shrinks to the neighbours of the best
    double lo = DM_U_LO, hi = DM_U_HI, D = 0.0;
    bool all_lo = true, all_hi = true;
#pragma unroll 1
    for (int round = 0; round < DM_ROUNDS; ++round) {
        const double step = (hi - lo) / 63.0;
        const double Dj = D_ref * exp2(lo + (double)lane * step);
        double c = dm_cost(R, Dj, dt, Rb, false, s0.uy, s0.ux).cost;
        int j = lane;
        tm_wave_argmin(c, j);
        all_lo = all_lo && j == 0;
        all_hi = all_hi && j == 63;
        D = __shfl(Dj, j, DM_THREADS);
        const int jl = j > 0 ? j - 1 : 0, jh = j < 63 ? j + 1 : 63;
        const double nlo = lo + (double)jl * step, nhi = lo + (double)jh * step;
        lo = nlo, hi = nhi;
    }
    int st = all_lo ? 2 : (all_hi ? 3 : 0);
    if (st == 2) D = 0.0;

    // log L at D and the observed information in ln D: lanes 0, 1, 2 take D, D e^h, D e^-h (the others repeat lane 0)
    const double Dl = lane == 1 ? D * TM_EXP_H : (lane == 2 ? D * TM_EXP_MH : D);
    const DmFit fit = dm_cost(R, Dl, dt, Rb, false, s0.uy, s0.ux);
    const double c0 = __shfl(fit.cost, 0, DM_THREADS), cp = __shfl(fit.cost, 1, DM_THREADS), cm = __shfl(fit.cost, 2, DM_THREADS);
    const double info = tm_curvature(cp, c0, cm);
    double sd = NAN;
    if (st != 2) {
        if (info > 0.0 && info < INFINITY)
            sd = D / sqrt(info);
        else if (st == 0)
            st = 4;
    }
    if (lane == 0) {
        const bool fine = c0 < INFINITY;                                  // the velocity stands where the cost at D is finite
        D_out[k] = D, D_std[k] = sd, loglik[k] = -0.5 * c0;
        v_out[2 * (int64_t)k] = fine ? fit.uy : NAN, v_out[2 * (int64_t)k + 1] = fine ? fit.ux : NAN;
        v_std[2 * (int64_t)k] = fine ? 1.0 / sqrt(fit.Cy) : NAN, v_std[2 * (int64_t)k + 1] = fine ? 1.0 / sqrt(fit.Cx) : NAN;
        n_increments[k] = n_inc, status[k] = st;
    }
}

// one THREAD per range: the same device function at the caller's parameters
__global__ __launch_bounds__(DM_THREADS) void dm_loglik_kernel(const double *__restrict__ pos, const double *__restrict__ var,
                                                               const int *__restrict__ frames, const unsigned char *__restrict__ use,
                                                               int N, const int *__restrict__ offsets, int n, double dt, double Rb,
                                                               const double *__restrict__ D, const double *__restrict__ v,
                                                               double *__restrict__ loglik, double *__restrict__ v_hat,
                                                               double *__restrict__ v_hat_std) {
    const int k = blockIdx.x * DM_THREADS + threadIdx.x;
    if (k >= n) return;
    TmRows R;
    R.pos = pos, R.var = var, R.frames = frames, R.use = use;
    tm_clamp_range(offsets, k, N, R.a, R.b);
    const double Dk = D[k];
    const bool given = v != nullptr;
    double gy, gx;
    bool fine = Dk >= 0.0 && Dk < INFINITY;
    if (given) {
        gy = v[2 * (int64_t)k], gx = v[2 * (int64_t)k + 1];
        fine = fine && tm_finite(gy) && tm_finite(gx);
    } else {
        const DmStart s0 = dm_start(R, dt);
        gy = s0.uy, gx = s0.ux;
    }
    const DmFit fit = dm_cost(R, Dk, dt, Rb, given, gy, gx);
    fine = fine && fit.cnt >= 2;
    loglik[k] = fine ? -0.5 * fit.cost : NAN;
    const bool has = fine && fit.cost < INFINITY;
    if (v_hat) v_hat[2 * (int64_t)k] = has ? fit.uy : NAN, v_hat[2 * (int64_t)k + 1] = has ? fit.ux : NAN;
    if (v_hat_std)
        v_hat_std[2 * (int64_t)k] = has ? 1.0 / sqrt(fit.Cy) : NAN, v_hat_std[2 * (int64_t)k + 1] = has ? 1.0 / sqrt(fit.Cx) : NAN;
}

}  // namespace

extern "C" int mivit_track_directed_ml(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                                       const int *offsets, int n, double dt, double R, double *D, double *D_std, double *v,
                                       double *v_std, double *loglik, int *n_increments, int *status, void *stream) {
    if (int rc = tm_check_rows("track_directed_ml", pos, N, offsets, n, dt)) return rc;
    MIVIT_CHECK(R >= 0.0 && R <= 0.25, "track_directed_ml: blur coefficient R = %g outside [0, 1/4]", R);
    if (n == 0) return 0;
    MIVIT_CHECK(D && D_std && v && v_std && loglik && n_increments && status, "track_directed_ml: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(dm_kernel, dim3((unsigned)n), dim3(DM_THREADS), 0, static_cast<hipStream_t>(stream), pos, var, frames, use,
                       N, offsets, dt, R, D, D_std, v, v_std, loglik, n_increments, status);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_track_directed_loglik(const double *pos, const double *var, const int *frames, const unsigned char *use,
                                           int N, const int *offsets, int n, double dt, double R, const double *D, const double *v,
                                           double *loglik, double *v_hat, double *v_hat_std, void *stream) {
    if (int rc = tm_check_rows("track_directed_loglik", pos, N, offsets, n, dt)) return rc;
    MIVIT_CHECK(R >= 0.0 && R <= 0.25, "track_directed_loglik: blur coefficient R = %g outside [0, 1/4]", R);
    if (n == 0) return 0;
    MIVIT_CHECK(D && loglik, "track_directed_loglik: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(dm_loglik_kernel, dim3((unsigned)((n + DM_THREADS - 1) / DM_THREADS)), dim3(DM_THREADS), 0,
                       static_cast<hipStream_t>(stream), pos, var, frames, use, N, offsets, n, dt, R, D, v, loglik, v_hat, v_hat_std);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
