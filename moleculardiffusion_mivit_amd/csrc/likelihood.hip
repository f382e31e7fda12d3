// Per-track maximum-likelihood diffusion coefficient with its standard error, from row positions that each carry their own
// variance (no counterpart in the reference).  The model is the exact Gaussian likelihood of a track's increments under
// localisation noise of known, row-dependent variance, motion blur and missing frames: Berglund, Phys. Rev. E 82, 011917
// (2010); Michalet & Berglund, Phys. Rev. E 85, 061916 (2012); Relich et al., Phys. Rev. E 93, 042401 (2016).
// include/mivit_hip.h spells the arithmetic out; helpers/msd._diffusion_ml_numpy restates it in numpy.
//
// ONE WAVE PER RANGE (a workgroup of 64 threads), lane j = candidate j of a fixed grid search over log2 D.  Every lane walks
// the same rows, so the row index, the usability test and the loop are wave-uniform (the compiler is free to fetch a row with
// scalar loads; where it does not, the 64 lanes read one address and the read is a broadcast) and only D differs between
// lanes.  The state of the LDL^T recurrence of the tridiagonal covariance (per axis the last pivot's reciprocal and the last
// residual, the running determinant and quadratic form) lives in registers: no LDS, no scratch, no atomics, no barrier, and a
// range has no maximum length.  The rows are read again from global memory in each of the 8 passes (one for D_ref, six rounds
// of the search, one for the three points of the curvature): a range is a few KiB and stays in cache, and staging it in LDS
// would put a limit on its length or a chunk loop with barriers around a recurrence that is bound by its division.
//
// The determinant is kept as a PRODUCT rescaled exactly (frexp: mantissa in [0.5, 1) and an integer exponent), not as a sum of
// logarithms: the inner loop has no log, one log per candidate and pass remains, and the restatement does the same in numpy,
// so the two differ in that log and in exp2 alone.  The arg-min goes through xor shuffles (least cost, lowest lane on a tie).
// The work of a range does not depend on where it sits in a batch: its outputs are bitwise the same alone, anywhere in a batch
// and in every launch.
//
// No contraction into FMA, as in segment.hip and hmm.hip.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int ML_THREADS = 64;                                            // one wave = the candidates of a round
constexpr int ML_ROUNDS = 6;
constexpr double ML_U_LO = -20.0, ML_U_HI = 4.0;                          // the first bracket of log2(D / D_ref)
constexpr double ML_LOG_2PI = 1.8378770664093453;                         // np.log(2 * np.pi)
constexpr double ML_LN2 = 0.6931471805599453;                             // np.log(2)
constexpr double ML_EXP_H = 1.0157477085866857;                           // np.exp(1 / 64): the step h in ln D of the curvature
constexpr double ML_EXP_MH = 0.9844964370054085;                          // np.exp(-1 / 64)
constexpr double ML_INV_2H2 = 2048.0;                                     // 1 / (2 h^2)

struct MlRows {
    const double *pos, *var;
    const int *frames;
    const unsigned char *use;
    int a, b;                                                             // the range, clamped into [0, N]
};

struct MlRow {
    double y, x, vy, vx;
    int f;
    bool ok;
};

__device__ __forceinline__ bool ml_finite(double v) { return fabs(v) < INFINITY; }

// row r of the range: usable when its flag is set, both coordinates are finite and both variances are finite and >= 0
__device__ __forceinline__ MlRow ml_row(const MlRows &R, int r) {
    MlRow w;
    w.y = R.pos[2 * (int64_t)r];
    w.x = R.pos[2 * (int64_t)r + 1];
    w.vy = R.var ? R.var[2 * (int64_t)r] : 0.0;
    w.vx = R.var ? R.var[2 * (int64_t)r + 1] : 0.0;
    w.f = R.frames ? R.frames[r] : r - R.a;
    w.ok = (R.use ? R.use[r] != 0 : true) && ml_finite(w.y) && ml_finite(w.x) && w.vy >= 0.0 && w.vy < INFINITY &&
           w.vx >= 0.0 && w.vx < INFINITY;
    return w;
}

// one axis of one increment: the pivot e and the residual z of the LDL^T recurrence, the quadratic form and the determinant
__device__ __forceinline__ void ml_axis(bool first, double base, double cR, double pv, double v, double d, double &rinv, double &z,
                                        double &Q, double &pm, int &pe, bool &bad) {
    const double a = (base + pv) + v;
    double e;
    if (first) {
        e = a;
        z = d;
    } else {
        const double b = cR - pv;                                         // pv: the variance of the row both increments share
        const double l = b * rinv;
        e = a - l * b;
        z = d - l * z;
    }
    if (!(e > 0.0)) bad = true;                                           // not positive definite (or NaN): the candidate is rejected
    rinv = 1.0 / e;
    Q = Q + (z * z) * rinv;
    int ex;
    pm = frexp(pm * e, &ex);
    pe += ex;
}

// -2 log L of the range at D (this lane's candidate); +inf for a rejected candidate and for a cost that is not a number
__device__ __forceinline__ double ml_cost(const MlRows &R, double D, double dt, double Rb) {
    const double c1 = (2.0 * D) * dt, cR = Rb * c1, tR = 2.0 * Rb;
    double py = 0.0, px = 0.0, pvy = 0.0, pvx = 0.0;
    double ry = 0.0, rx = 0.0, zy = 0.0, zx = 0.0, Q = 0.0, pm = 0.5;
    int pf = 0, cnt = 0, pe = 1;
    bool bad = false;
    for (int r = R.a; r < R.b; ++r) {
        const MlRow w = ml_row(R, r);
        if (!w.ok) continue;                                              // wave-uniform
        if (cnt > 0) {
            const double base = c1 * ((double)(w.f - pf) - tR);
            ml_axis(cnt == 1, base, cR, pvy, w.vy, w.y - py, ry, zy, Q, pm, pe, bad);
            ml_axis(cnt == 1, base, cR, pvx, w.vx, w.x - px, rx, zx, Q, pm, pe, bad);
        }
        py = w.y, px = w.x, pvy = w.vy, pvx = w.vx, pf = w.f;
        ++cnt;
    }
    const double cost = ((log(pm) + (double)pe * ML_LN2) + Q) + (double)(2 * (cnt - 1)) * ML_LOG_2PI;
    return (bad || !(cost < INFINITY)) ? INFINITY : cost;
}

__global__ __launch_bounds__(ML_THREADS) void ml_kernel(const double *__restrict__ pos, const double *__restrict__ var,
                                                        const int *__restrict__ frames, const unsigned char *__restrict__ use,
                                                        int N, const int *__restrict__ offsets, double dt, double Rb,
                                                        double *__restrict__ D_out, double *__restrict__ D_std,
                                                        double *__restrict__ loglik, int *__restrict__ n_increments,
                                                        int *__restrict__ status) {
    const int k = blockIdx.x, lane = threadIdx.x;
    MlRows R;
    R.pos = pos, R.var = var, R.frames = frames, R.use = use;
    int a = offsets[k], b = offsets[k + 1];
    a = a < 0 ? 0 : (a > N ? N : a);                                      // never read outside [0, N), whatever offsets holds
    b = b < a ? a : (b > N ? N : b);
    R.a = a, R.b = b;

    // pass 0: the usable rows, D_ref = sum d^2 (both axes) / (4 dt sum g); the same in every lane
    double S = 0.0, py = 0.0, px = 0.0;
    int64_t G = 0;
    int pf = 0, cnt = 0;
    for (int r = a; r < b; ++r) {
        const MlRow w = ml_row(R, r);
        if (!w.ok) continue;
        if (cnt > 0) {
            const double dy = w.y - py, dx = w.x - px;
            S = S + (dy * dy + dx * dx);
            G += w.f - pf;
        }
        py = w.y, px = w.x, pf = w.f;
        ++cnt;
    }
    const int n_inc = cnt > 0 ? cnt - 1 : 0;
    if (n_inc < 2) {                                                      // wave-uniform
        if (lane == 0) {
            D_out[k] = NAN, D_std[k] = NAN, loglik[k] = NAN;
            n_increments[k] = n_inc, status[k] = 1;
        }
        return;
    }
    const double D_ref = S / ((4.0 * dt) * (double)G);

    // the search: 64 candidates over the bracket, the bracket shrinks to the neighbours of the best
    double lo = ML_U_LO, hi = ML_U_HI, D = 0.0;
    bool all_lo = true, all_hi = true;
#pragma unroll 1
    for (int round = 0; round < ML_ROUNDS; ++round) {
        const double step = (hi - lo) / 63.0;
        const double Dj = D_ref * exp2(lo + (double)lane * step);
        double c = ml_cost(R, Dj, dt, Rb);
        int j = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                                // every lane ends with the least cost and its lowest lane
            const double oc = __shfl_xor(c, o, ML_THREADS);
            const int oj = __shfl_xor(j, o, ML_THREADS);
            if (oc < c || (oc == c && oj < j)) c = oc, j = oj;
        }
        all_lo = all_lo && j == 0;
        all_hi = all_hi && j == 63;
        D = __shfl(Dj, j, ML_THREADS);
        const int jl = j > 0 ? j - 1 : 0, jh = j < 63 ? j + 1 : 63;
        const double nlo = lo + (double)jl * step, nhi = lo + (double)jh * step;
        lo = nlo, hi = nhi;
    }
    int st = all_lo ? 2 : (all_hi ? 3 : 0);
    if (st == 2) D = 0.0;

    // log L at D and the observed information in ln D: lanes 0, 1, 2 take D, D e^h, D e^-h (the others repeat lane 0)
    const double Dl = lane == 1 ? D * ML_EXP_H : (lane == 2 ? D * ML_EXP_MH : D);
    const double c = ml_cost(R, Dl, dt, Rb);
    const double c0 = __shfl(c, 0, ML_THREADS), cp = __shfl(c, 1, ML_THREADS), cm = __shfl(c, 2, ML_THREADS);
    const double info = ((cp - c0) + (cm - c0)) * ML_INV_2H2;
    double sd = NAN;
    if (st != 2) {
        if (info > 0.0 && info < INFINITY)
            sd = D / sqrt(info);
        else if (st == 0)
            st = 4;
    }
    if (lane == 0) {
        D_out[k] = D, D_std[k] = sd, loglik[k] = -0.5 * c0;
        n_increments[k] = n_inc, status[k] = st;
    }
}

}  // namespace

extern "C" int mivit_track_diffusion_ml(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                                        const int *offsets, int n, double dt, double R, double *D, double *D_std, double *loglik,
                                        int *n_increments, int *status, void *stream) {
    MIVIT_CHECK(N >= 0 && n >= 0, "track_diffusion_ml: N = %d, n = %d: negative size", N, n);
    MIVIT_CHECK(dt > 0.0 && dt < INFINITY, "track_diffusion_ml: dt = %g must be positive and finite", dt);
    MIVIT_CHECK(R >= 0.0 && R <= 0.25, "track_diffusion_ml: blur coefficient R = %g outside [0, 1/4]", R);
    if (n == 0) return 0;
    MIVIT_CHECK(offsets && D && D_std && loglik && n_increments && status, "track_diffusion_ml: null pointer");
    MIVIT_CHECK(pos || N == 0, "track_diffusion_ml: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(ml_kernel, dim3((unsigned)n), dim3(ML_THREADS), 0, static_cast<hipStream_t>(stream), pos, var, frames, use,
                       N, offsets, dt, R, D, D_std, loglik, n_increments, status);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
