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
// and in every launch.  The rows, the reference scale, the product and the arg-min are those of track_ml.h.
//
// No contraction into FMA, as in segment.hip and hmm.hip.
#pragma clang fp contract(off)

#include "track_ml.h"

namespace {

constexpr int ML_THREADS = TM_WAVE;                                       // one wave = the candidates of a round
constexpr int ML_ROUNDS = 6;
constexpr double ML_U_LO = -20.0, ML_U_HI = 4.0;                          // the first bracket of log2(D / D_ref)

// one axis of one increment: the pivot e and the residual z of the LDL^T recurrence, the quadratic form and the determinant
__device__ __forceinline__ void ml_axis(bool first, double base, double cR, double pv, double v, double d, double &rinv, double &z,
                                        double &Q, TmProd &det, bool &bad) {
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
    det.mul(e);
}

// -2 log L of the range at D (this lane's candidate); +inf for a rejected candidate and for a cost that is not a number
__device__ __forceinline__ double ml_cost(const TmRows &R, double D, double dt, double Rb) {
    const double c1 = (2.0 * D) * dt, cR = Rb * c1, tR = 2.0 * Rb;
    double py = 0.0, px = 0.0, pvy = 0.0, pvx = 0.0;
    double ry = 0.0, rx = 0.0, zy = 0.0, zx = 0.0, Q = 0.0;
    TmProd det;
    int pf = 0, cnt = 0;
    bool bad = false;
    for (int r = R.a; r < R.b; ++r) {
        const TmRow w = tm_row(R, r);
        if (!w.ok) continue;                                              // wave-uniform
        if (cnt > 0) {
            const double base = c1 * ((double)(w.f - pf) - tR);
            ml_axis(cnt == 1, base, cR, pvy, w.vy, w.y - py, ry, zy, Q, det, bad);
            ml_axis(cnt == 1, base, cR, pvx, w.vx, w.x - px, rx, zx, Q, det, bad);
        }
        py = w.y, px = w.x, pvy = w.vy, pvx = w.vx, pf = w.f;
        ++cnt;
    }
    return tm_finish_cost(det, Q, cnt - 1, bad);
}

__global__ __launch_bounds__(ML_THREADS) void ml_kernel(const double *__restrict__ pos, const double *__restrict__ var,
                                                        const int *__restrict__ frames, const unsigned char *__restrict__ use,
                                                        int N, const int *__restrict__ offsets, double dt, double Rb,
                                                        double *__restrict__ D_out, double *__restrict__ D_std,
                                                        double *__restrict__ loglik, int *__restrict__ n_increments,
                                                        int *__restrict__ status) {
    const int k = blockIdx.x, lane = threadIdx.x;
    TmRows R;
    R.pos = pos, R.var = var, R.frames = frames, R.use = use;
    tm_clamp_range(offsets, k, N, R.a, R.b);

    // pass 0: the usable rows and D_ref; the same in every lane
    const TmScale sc = tm_scale(R);
    const int n_inc = sc.n_inc();
    if (n_inc < 2) {                                                      // wave-uniform
        if (lane == 0) {
            D_out[k] = NAN, D_std[k] = NAN, loglik[k] = NAN;
            n_increments[k] = n_inc, status[k] = 1;
        }
        return;
    }
    const double D_ref = tm_d_ref(sc.S, dt, sc.G);

    // the search: 64 candidates over the bracket, the bracket shrinks to the neighbours of the best
    double lo = ML_U_LO, hi = ML_U_HI, D = 0.0;
    bool all_lo = true, all_hi = true;
#pragma unroll 1
    for (int round = 0; round < ML_ROUNDS; ++round) {
        const double step = (hi - lo) / 63.0;
        const double Dj = D_ref * exp2(lo + (double)lane * step);
        double c = ml_cost(R, Dj, dt, Rb);
        int j = lane;
        tm_wave_argmin(c, j);
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
    const double Dl = lane == 1 ? D * TM_EXP_H : (lane == 2 ? D * TM_EXP_MH : D);
    const double c = ml_cost(R, Dl, dt, Rb);
    const double c0 = __shfl(c, 0, ML_THREADS), cp = __shfl(c, 1, ML_THREADS), cm = __shfl(c, 2, ML_THREADS);
    const double info = tm_curvature(cp, c0, cm);
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
    if (int rc = tm_check_rows("track_diffusion_ml", pos, N, offsets, n, dt)) return rc;
    MIVIT_CHECK(R >= 0.0 && R <= 0.25, "track_diffusion_ml: blur coefficient R = %g outside [0, 1/4]", R);
    if (n == 0) return 0;
    MIVIT_CHECK(D && D_std && loglik && n_increments && status, "track_diffusion_ml: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(ml_kernel, dim3((unsigned)n), dim3(ML_THREADS), 0, static_cast<hipStream_t>(stream), pos, var, frames, use,
                       N, offsets, dt, R, D, D_std, loglik, n_increments, status);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
