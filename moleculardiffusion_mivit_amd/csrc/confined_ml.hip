// Per-track maximum-likelihood confinement radius with error bars, and the exact log-likelihood of confined diffusion at given
// parameters, from row positions that each carry their own variance (no counterpart in the reference).  The model is an
// isotropic Ornstein-Uhlenbeck process (diffusion in a harmonic well) seen at instantaneous exposure (motion blur is NOT
// modelled) through Gaussian noise of known, row-dependent variance, with frames that may be missing.  Its exact likelihood is
// a scalar Kalman filter per axis, conditioned on the first usable row, linear in the centre of the well, which is therefore
// profiled out in closed form.  include/mivit_hip.h spells the arithmetic out; helpers/msd._confined_ml_numpy restates it.
//
// ONE WAVE PER RANGE (a workgroup of 64 threads), lane 8 i + j = candidate (D_i, s2_j) of a fixed 8 x 8 grid search over
// (log2 D, log2 s2): every lane walks the same rows, so the row index, the usability test and the loop
// are wave-uniform and only the two parameters differ between lanes.  The filter's state of both axes (mean as a + b c,
// variance, three sums of the normal equation of the centre), the determinant and the parameters are about 20 doubles a
// lane and live in registers: no LDS, no scratch, no atomics, no barrier, and a range has no maximum length.  The rows are
// read again from global memory in each of the 23 passes (two for the reference scales, 20 rounds, one for the stencil of
// the curvature); a range is a few KiB and stays in cache.
//
// The determinant is a PRODUCT rescaled exactly by frexp: no log in the loop.  The arg-min goes through
// xor shuffles (least cost, lowest lane on a tie).  The work of a range does not depend on where it sits in a batch: its
// outputs are bitwise the same alone, anywhere in a batch and in every launch.  The rows, the reference scale D_ref, the
// product, the arg-min and the stencil's information matrix are those of track_ml.h.
//
// No contraction into FMA.
#pragma clang fp contract(off)

#include "track_ml.h"

namespace {

constexpr int CF_THREADS = TM_WAVE;                                       // one wave = the 8 x 8 candidates of a round
constexpr int CF_ROUNDS = 20;
constexpr int CF_MIN_INCREMENTS = 4;
constexpr double CF_U_LO = -12.0, CF_U_HI = 4.0;                          // the first bracket of log2(D / D_ref)
constexpr double CF_W_LO = -6.0, CF_W_HI = 18.0;                          // the first bracket of log2(s2 / S_ref)
constexpr double CF_FAST = 4.0;                                           // status 3 where lambda dt is above it

struct CfFit {
    double cost, cy, cx, hy, hx;                                          // -2 log L, the centre, Shh per axis
    int cnt;                                                              // usable rows
};

// one axis of one row: predict over the gap, the innovation and its variance, the sums of the centre's normal equation, update
__device__ __forceinline__ void cf_axis(double phi, double om, double q, double y, double v, double &a, double &b, double &P,
                                        double &Syy, double &Syh, double &Shh, TmProd &det, bool &bad) {
    const double Pm = (phi * phi) * P + q;
    const double F = Pm + v;
    if (!(F > 0.0)) bad = true;                                           // not positive (or NaN): the candidate is rejected
    const double r = 1.0 / F;
    const double am = phi * a;
    const double eh = phi * b + om;
    const double ey = y - am;
    const double K = Pm * r;
    a = am + K * ey;
    b = eh - K * eh;
    P = (1.0 - K) * Pm;
    Syy = Syy + (ey * ey) * r;
    Syh = Syh + (ey * eh) * r;
    Shh = Shh + (eh * eh) * r;
    det.mul(F);
}

// -2 log L of the range at (D, s2), this lane's candidate, with the centre (gy, gx) where `given`, else profiled; +inf for a
// rejected candidate and for a cost that is not a number
__device__ __forceinline__ CfFit cf_cost(const TmRows &R, double D, double s2, double dt, bool given, double gy, double gx) {
    const double ldt = (D / s2) * dt;
    double ay = 0.0, by = 0.0, Py = 0.0, ax = 0.0, bx = 0.0, Px = 0.0;
    double Syy_y = 0.0, Syh_y = 0.0, Shh_y = 0.0, Syy_x = 0.0, Syh_x = 0.0, Shh_x = 0.0;
    TmProd det;
    int pf = 0, cnt = 0;
    bool bad = false;
    for (int r = R.a; r < R.b; ++r) {
        const TmRow w = tm_row(R, r);
        if (!w.ok) continue;                                              // wave-uniform
        if (cnt == 0) {
            ay = w.y, Py = w.vy, ax = w.x, Px = w.vx;                     // conditioned on the first usable row
        } else {
            const double t = ldt * (double)(w.f - pf);
            const double om = -expm1(-t);
            const double phi = 1.0 - om;
            const double q = s2 * (-expm1(-(2.0 * t)));
            cf_axis(phi, om, q, w.y, w.vy, ay, by, Py, Syy_y, Syh_y, Shh_y, det, bad);
            cf_axis(phi, om, q, w.x, w.vx, ax, bx, Px, Syy_x, Syh_x, Shh_x, det, bad);
        }
        pf = w.f;
        ++cnt;
    }
    CfFit fit;
    double Qy, Qx;
    if (given) {
        fit.cy = gy, fit.cx = gx;
        Qy = (Syy_y - ((2.0 * gy) * Syh_y)) + (gy * gy) * Shh_y;
        Qx = (Syy_x - ((2.0 * gx) * Syh_x)) + (gx * gx) * Shh_x;
    } else {
        fit.cy = Shh_y > 0.0 ? Syh_y / Shh_y : NAN;
        fit.cx = Shh_x > 0.0 ? Syh_x / Shh_x : NAN;
        Qy = Shh_y > 0.0 ? Syy_y - (Syh_y * Syh_y) / Shh_y : Syy_y;
        Qx = Shh_x > 0.0 ? Syy_x - (Syh_x * Syh_x) / Shh_x : Syy_x;
    }
    fit.cost = tm_finish_cost(det, Qy + Qx, cnt - 1, bad);
    fit.hy = Shh_y, fit.hx = Shh_x, fit.cnt = cnt;
    return fit;
}

__device__ __forceinline__ double cf_stencil_factor(int i) { return i == 0 ? TM_EXP_MH : (i == 1 ? 1.0 : TM_EXP_H); }

struct CfOut {
    double *D, *D_std, *radius, *radius_std, *lambda, *lambda_std, *corr, *centre, *centre_std, *loglik;
    int *n_increments, *status;
};

__global__ __launch_bounds__(CF_THREADS) void cf_kernel(const double *__restrict__ pos, const double *__restrict__ var,
                                                        const int *__restrict__ frames, const unsigned char *__restrict__ use,
                                                        int N, const int *__restrict__ offsets, double dt, CfOut out) {
    const int k = blockIdx.x, lane = threadIdx.x;
    TmRows R;
    R.pos = pos, R.var = var, R.frames = frames, R.use = use;
    tm_clamp_range(offsets, k, N, R.a, R.b);

    // pass 0: the usable rows, D_ref and the sums of the positions; the same in every lane
    const TmScale sc = tm_scale(R);
    const int n_inc = sc.n_inc(), cnt = sc.cnt;
    if (n_inc < CF_MIN_INCREMENTS) {                                      // wave-uniform
        if (lane == 0) {
            out.D[k] = NAN, out.D_std[k] = NAN, out.radius[k] = NAN, out.radius_std[k] = NAN, out.lambda[k] = NAN;
            out.lambda_std[k] = NAN, out.corr[k] = NAN, out.loglik[k] = NAN;
            out.centre[2 * (int64_t)k] = NAN, out.centre[2 * (int64_t)k + 1] = NAN;
            out.centre_std[2 * (int64_t)k] = NAN, out.centre_std[2 * (int64_t)k + 1] = NAN;
            out.n_increments[k] = n_inc, out.status[k] = 1;
        }
        return;
    }
    const double D_ref = tm_d_ref(sc.S, dt, sc.G);
    // pass 0, second half: S_ref, half the summed variance of the usable positions about their mean
    const double my = sc.sy / (double)cnt, mx = sc.sx / (double)cnt;
    double ss = 0.0;
    for (int r = R.a; r < R.b; ++r) {
        const TmRow w = tm_row(R, r);
        if (!w.ok) continue;
        const double dy = w.y - my, dx = w.x - mx;
        ss = ss + (dy * dy + dx * dx);
    }
    const double S_ref = ss / (2.0 * (double)cnt);

    // the search: 8 x 8 candidates over the brackets, which shrink to the best candidate +- 2 cells (not clamped)
    double ulo = CF_U_LO, uhi = CF_U_HI, wlo = CF_W_LO, whi = CF_W_HI, ub = 0.0, wb = 0.0;
    bool u_lo = true, u_hi = true, w_lo = true;
    const double li = (double)(lane >> 3), lj = (double)(lane & 7);
#pragma unroll 1
    for (int round = 0; round < CF_ROUNDS; ++round) {
        const double su = (uhi - ulo) / 7.0, sw = (whi - wlo) / 7.0;
        const double Dj = D_ref * exp2(ulo + li * su), Sj = S_ref * exp2(wlo + lj * sw);
        double c = cf_cost(R, Dj, Sj, dt, false, 0.0, 0.0).cost;
        int j = lane;
        tm_wave_argmin(c, j);
        const int bi = j >> 3, bj = j & 7;
        ub = ulo + (double)bi * su, wb = wlo + (double)bj * sw;
        ulo = ub - 2.0 * su, uhi = ub + 2.0 * su, wlo = wb - 2.0 * sw, whi = wb + 2.0 * sw;
        u_lo = u_lo && bi == 0, u_hi = u_hi && bi == 7, w_lo = w_lo && bj == 0;
    }
    const double D = D_ref * exp2(ub), s2 = S_ref * exp2(wb);
    const double lam = D / s2;
    int st = wb >= CF_W_HI ? 2 : (lam * dt > CF_FAST ? 3 : ((u_lo || u_hi || w_lo) ? 5 : 0));

    // the 3 x 3 stencil in (ln D, ln s2): lane 3 a + b takes (D e^{(a - 1) h}, s2 e^{(b - 1) h}), lanes 9 .. 63 repeat lane 0
    const int sl = lane < 9 ? lane : 0;
    const CfFit fit = cf_cost(R, D * cf_stencil_factor(sl / 3), s2 * cf_stencil_factor(sl % 3), dt, false, 0.0, 0.0);
    double c[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) c[i] = __shfl(fit.cost, i, CF_THREADS);
    const double cy = __shfl(fit.cy, 4, CF_THREADS), cx = __shfl(fit.cx, 4, CF_THREADS);
    const double hy = __shfl(fit.hy, 4, CF_THREADS), hx = __shfl(fit.hx, 4, CF_THREADS);
    const double c0 = c[4];
    const TmHess2 H(c);                                                   // u = ln D, v = ln s2
    const double Hdd = H.uu, Hss = H.vv, Hds = H.uv, det = H.det;
    if (!(c0 < INFINITY)) st = 4;                                         // no candidate was accepted
    const bool pd = H.pd();
    if (!pd && st == 0) st = 4;
    const bool full = pd && (st == 0 || st == 5);
    if (lane == 0) {
        const double radius = sqrt(2.0 * s2);
        const double vl = ((Hss + Hdd) + 2.0 * Hds) / det;
        out.D[k] = D;
        out.loglik[k] = -0.5 * c0;
        out.D_std[k] = full ? D * sqrt(Hss / det) : NAN;
        out.radius[k] = st == 2 ? INFINITY : radius;
        out.radius_std[k] = full ? (0.5 * radius) * sqrt(Hdd / det)
                                 : ((st == 3 && Hss > 0.0 && Hss < INFINITY) ? (0.5 * radius) / sqrt(Hss) : NAN);
        out.lambda[k] = st == 2 ? 0.0 : lam;
        out.lambda_std[k] = (full && vl >= 0.0) ? lam * sqrt(vl) : NAN;
        out.corr[k] = full ? -Hds / sqrt(Hdd * Hss) : NAN;
        out.centre[2 * (int64_t)k] = st != 2 ? cy : NAN;
        out.centre[2 * (int64_t)k + 1] = st != 2 ? cx : NAN;
        out.centre_std[2 * (int64_t)k] = (st != 2 && st != 4 && hy > 0.0) ? 1.0 / sqrt(hy) : NAN;
        out.centre_std[2 * (int64_t)k + 1] = (st != 2 && st != 4 && hx > 0.0) ? 1.0 / sqrt(hx) : NAN;
        out.n_increments[k] = n_inc, out.status[k] = st;
    }
}

// one THREAD per range: the same device function at the caller's parameters
__global__ __launch_bounds__(CF_THREADS) void cf_loglik_kernel(const double *__restrict__ pos, const double *__restrict__ var,
                                                               const int *__restrict__ frames, const unsigned char *__restrict__ use,
                                                               int N, const int *__restrict__ offsets, int n, double dt,
                                                               const double *__restrict__ D, const double *__restrict__ s2,
                                                               const double *__restrict__ centre, double *__restrict__ loglik) {
    const int k = blockIdx.x * CF_THREADS + threadIdx.x;
    if (k >= n) return;
    TmRows R;
    R.pos = pos, R.var = var, R.frames = frames, R.use = use;
    tm_clamp_range(offsets, k, N, R.a, R.b);
    const double Dk = D[k], Sk = s2[k];
    const bool given = centre != nullptr;
    const CfFit fit = cf_cost(R, Dk, Sk, dt, given, given ? centre[2 * (int64_t)k] : 0.0, given ? centre[2 * (int64_t)k + 1] : 0.0);
    const bool fine = fit.cnt >= 2 && Dk > 0.0 && Dk < INFINITY && Sk > 0.0 && Sk < INFINITY;
    loglik[k] = fine ? -0.5 * fit.cost : NAN;
}

}  // namespace

extern "C" int mivit_track_confined_ml(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                                       const int *offsets, int n, double dt, double *D, double *D_std, double *radius,
                                       double *radius_std, double *lambda, double *lambda_std, double *corr, double *centre,
                                       double *centre_std, double *loglik, int *n_increments, int *status, void *stream) {
    if (int rc = tm_check_rows("track_confined_ml", pos, N, offsets, n, dt)) return rc;
    if (n == 0) return 0;
    MIVIT_CHECK(D && D_std && radius && radius_std && lambda && lambda_std && corr && centre && centre_std && loglik &&
                    n_increments && status,
                "track_confined_ml: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    const CfOut out{D, D_std, radius, radius_std, lambda, lambda_std, corr, centre, centre_std, loglik, n_increments, status};
    hipLaunchKernelGGL(cf_kernel, dim3((unsigned)n), dim3(CF_THREADS), 0, static_cast<hipStream_t>(stream), pos, var, frames, use,
                       N, offsets, dt, out);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_track_confined_loglik(const double *pos, const double *var, const int *frames, const unsigned char *use,
                                           int N, const int *offsets, int n, double dt, const double *D, const double *s2,
                                           const double *centre, double *loglik, void *stream) {
    if (int rc = tm_check_rows("track_confined_loglik", pos, N, offsets, n, dt)) return rc;
    if (n == 0) return 0;
    MIVIT_CHECK(D && s2 && loglik, "track_confined_loglik: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(cf_loglik_kernel, dim3((unsigned)((n + CF_THREADS - 1) / CF_THREADS)), dim3(CF_THREADS), 0,
                       static_cast<hipStream_t>(stream), pos, var, frames, use, N, offsets, n, dt, D, s2, centre, loglik);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
