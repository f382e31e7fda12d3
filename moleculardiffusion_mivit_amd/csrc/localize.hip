// Poisson maximum-likelihood fit of every localisation of a movie with a Cramer-Rao bound per parameter: Smith, Joseph,
// Rieger & Lidke, Nat. Methods 7, 373 (2010) with the Levenberg-Marquardt form of Laurence & Chromy, Nat. Methods 7, 338
// (2010) and the readout variance added to data and model as Huang et al., Nat. Methods 10, 653 (2013) do.  The least-squares
// fit it stands beside is csrc/tracking.hip::rg_kernel; the damped loop (lambda schedule, stopping rule, status codes, and the
// cost slack, taken here of the magnitude of the summed terms) is the one csrc/spot_fit.h::sf_damped_fit describes, written out
// here with its own factorisation because this kernel measured about 1 % slower on the shared templates: a change
// to the loop is made there, here and in rg_kernel.  The cost, gradient and matrix are the Poisson ones.
//
// Model of a patch [P, P] with pixel centres at integers, p = (N photons, x0, y0, s, b):
//   mu(iy, ix) = b + N E(ix; x0, s) E(iy; y0, s) + read_var,   E(i; c, s) = 1/2 [erf((i + 1/2 - c) / (sqrt(2) s)) - erf((i - 1/2 - c) / (sqrt(2) s))]
// Data d = max((patch - offset) / gain, 0) + read_var.  Cost: the Poisson deviance 2 sum(mu - d + d log(d / mu)); gradient
// sum (1 - d / mu) dmu; matrix: the Fisher information sum dmu dmu^T / mu.
//
// One thread per patch, fp64 (as rg_kernel, and for its reason: a movie yields thousands of patches, the loop is serial, no
// cross-lane order has to be pinned).  The model is separable: an evaluation fills six per-axis tables (E, dE/dc, dE/ds for x
// and for y) from 2 (P + 1) erf and 2 (P + 1) exp, then the P^2 pixels are multiply-adds into the 15 matrix entries.  The
// pixel loop indexes the tables at run time, which would send a private array to scratch, so they live in LDS as
// [table][k][lane]: 6 P doubles per lane, 46 080 bytes for a wave at P = 15, sized to P and to the lanes at launch; lane-
// contiguous, so every read is conflict-free, and only the owning lane touches an entry, so no barrier is needed.  The patch
// itself is re-read from global memory in every evaluation (each lane's P^2 floats are contiguous); staging it in LDS was
// measured and is a third slower at 10^6 patches, for the waves it takes from a CU (MIVIT_ML_STAGE_PATCH below).
//
// fit_sigma = 0 holds s at sigma0: the dE/ds tables are zero and the matrix gets a 1 on the diagonal of s, so the five-by-five
// Cholesky factor is the four-by-four one with a row of zeros added, term by term, and the step of s is exactly 0.
//
// No contraction into FMA: the host restatement (helpers/tracking._fit_mle_numpy) differs by erf, exp and log alone.
#pragma clang fp contract(off)

#include "common.h"
#include "spot_fit.h"

namespace {

// A/B switch, measurement only: -DMIVIT_ML_STAGE_PATCH copies each lane's raw patch into LDS once, as [pixel][lane]
// floats behind the tables, and every evaluation reads it from there; the arithmetic, and so every bit of the result, is the
// same.  It needs 4 P^2 more bytes per lane, which passes 64 KiB a wave above P = 11: such a build refuses larger patches.
#ifdef MIVIT_ML_STAGE_PATCH
#define ML_PIXEL(patch, t, L) (patch)[(t) * (L)]
#else
#define ML_PIXEL(patch, t, L) (patch)[t]
#endif

struct Fisher {
    double cost;              // the deviance
    double mag;               // 2 sum(mu + d): what the rounding error of the deviance scales with
    double g[5];              // sum (1 - d / mu) dmu
    double A[15];             // sum dmu dmu^T / mu, lower triangle row by row: A[i (i + 1) / 2 + j], j <= i
    bool bad;                 // outside the model's domain: N <= 0, s outside (0.2, P), or a pixel with mu <= 0
};

// the three tables of one axis for the centre c: tab[k L] = E(k), tab[(P + k) L] = dE/dc, tab[(2 P + k) L] = dE/ds (0 with fs = 0)
__device__ void ml_axis(double *tab, int L, int P, double c, double s, bool fs) {
    const double w = SF_SQRT2 * s, nc = 1.0 / (SF_SQRT_2PI * s), ns = nc / s;
    double t0 = (0.0 - 0.5) - c;
    double u = t0 / w;
    double e0 = erf(u), g0 = exp(-(u * u));
    for (int k = 0; k < P; ++k) {
        const double t1 = ((double)(k + 1) - 0.5) - c;
        u = t1 / w;
        const double e1 = erf(u), g1 = exp(-(u * u));
        tab[k * L] = 0.5 * (e1 - e0);
        tab[(P + k) * L] = (g0 - g1) * nc;
        tab[(2 * P + k) * L] = fs ? (t0 * g0 - t1 * g1) * ns : 0.0;
        t0 = t1;
        e0 = e1;
        g0 = g1;
    }
}

__device__ void ml_eval(const float *patch, int P, const Camera &cam, const double *p, bool fs, double *tab, int L, Fisher &n) {
    n.cost = 0.0;
    n.mag = 0.0;
    for (int i = 0; i < 5; ++i) n.g[i] = 0.0;
    for (int i = 0; i < 15; ++i) n.A[i] = 0.0;
    n.bad = !(p[0] > 0.0) || !(p[3] > SF_MIN_SIGMA) || !(p[3] < (double)P);
    if (n.bad) return;
    double *tx = tab, *ty = tab + 3 * P * L;
    ml_axis(tx, L, P, p[1], p[3], fs);
    ml_axis(ty, L, P, p[2], p[3], fs);
    bool bad = false;
    for (int iy = 0; iy < P; ++iy) {
        const double Ey = ty[iy * L];
        const double nEy = p[0] * Ey, ndEy = p[0] * ty[(P + iy) * L], nsEy = p[0] * ty[(2 * P + iy) * L];
        for (int ix = 0; ix < P; ++ix) {
            const double Ex = tx[ix * L], dEx = tx[(P + ix) * L], sEx = tx[(2 * P + ix) * L];
            const double mu = (p[4] + nEy * Ex) + cam.read_var;
            bad = bad || !(mu > 0.0);
            const double d = sf_data(ML_PIXEL(patch, iy * P + ix, L), cam);
            const double rm = 1.0 / mu, r = d * rm;
            n.cost = n.cost + (d > 0.0 ? (mu - d) + d * log(r) : mu);
            n.mag = n.mag + (mu + d);
            const double J[5] = {Ex * Ey, nEy * dEx, ndEy * Ex, nEy * sEx + nsEy * Ex, 1.0};
            const double w = 1.0 - r;
            for (int i = 0; i < 5; ++i) {
                n.g[i] = n.g[i] + J[i] * w;
                const double Jr = J[i] * rm;
                for (int j = 0; j <= i; ++j) n.A[i * (i + 1) / 2 + j] = n.A[i * (i + 1) / 2 + j] + Jr * J[j];
            }
        }
    }
    n.cost = 2.0 * n.cost;
    n.mag = 2.0 * n.mag;
    if (!fs) n.A[3 * 4 / 2 + 3] = 1.0;
    n.bad = bad;
}

// Cholesky factor of A + lambda diag(A); false if the matrix is not positive definite (or not finite)
__device__ bool ml_chol(const Fisher &n, double lambda, double *L) {
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = n.A[i * (i + 1) / 2 + j];
            if (i == j) s = s + lambda * s;
            for (int k = 0; k < j; ++k) s = s - L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            if (i == j) {
                if (!(s > 0.0) || !(s < 1e300)) return false;
                L[i * (i + 1) / 2 + i] = sqrt(s);
            } else {
                L[i * (i + 1) / 2 + j] = s / L[j * (j + 1) / 2 + j];
            }
        }
    return true;
}

// solves (A + lambda diag(A)) d = -g
__device__ bool ml_solve(const Fisher &n, double lambda, double *d) {
    double L[15];
    if (!ml_chol(n, lambda, L)) return false;
    double z[5];
    for (int i = 0; i < 5; ++i) {
        double s = -n.g[i];
        for (int k = 0; k < i; ++k) s = s - L[i * (i + 1) / 2 + k] * z[k];
        z[i] = s / L[i * (i + 1) / 2 + i];
    }
    for (int i = 4; i >= 0; --i) {
        double s = z[i];
        for (int k = i + 1; k < 5; ++k) s = s - L[k * (k + 1) / 2 + i] * d[k];
        d[i] = s / L[i * (i + 1) / 2 + i];
    }
    return true;
}

// diagonal of A^-1 = L^-T L^-1: column j of X = L^-1 by forward substitution, v[j] = sum_i X[i][j]^2
__device__ bool ml_crlb(const Fisher &n, double *v) {
    double L[15];
    if (!ml_chol(n, 0.0, L)) return false;
    for (int j = 0; j < 5; ++j) {
        double X[5];
        X[j] = 1.0 / L[j * (j + 1) / 2 + j];
        double acc = X[j] * X[j];
        for (int i = j + 1; i < 5; ++i) {
            double s = 0.0;
            for (int k = j; k < i; ++k) s = s - L[i * (i + 1) / 2 + k] * X[k];
            X[i] = s / L[i * (i + 1) / 2 + i];
            acc = acc + X[i] * X[i];
        }
        v[j] = acc;
    }
    return true;
}

__global__ __launch_bounds__(64) void ml_kernel(const float *__restrict__ patches, int N, int P, Camera cam, double sigma0,
                                                int fit_sigma, double xtol, double *params, double *crlb, double *deviance,
                                                int *status, int *iterations) {
    extern __shared__ double ml_tab[];                                    // [6][P][blockDim.x]
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int L = blockDim.x;
    double *tab = ml_tab + threadIdx.x;
    const bool fs = fit_sigma != 0;
    const float *patch = patches + (int64_t)i * P * P;
#ifdef MIVIT_ML_STAGE_PATCH
    float *stage = reinterpret_cast<float *>(ml_tab + 6 * P * L) + threadIdx.x;
#endif
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    bool finite = true;
    double mx = sf_data(patch[0], cam), mn = mx, sum = 0.0;
    for (int t = 0; t < P * P; ++t) {
        const float v = patch[t];
        finite = finite && (v - v == 0.f);
#ifdef MIVIT_ML_STAGE_PATCH
        stage[t * L] = v;
#endif
        const double d = sf_data(v, cam);
        mx = d > mx ? d : mx;
        mn = d < mn ? d : mn;
        sum = sum + d;
    }
    // start: background = the smallest pixel (at least 1e-3 of the largest), photons = what lies above it
    const double b0 = fmax(mn, 1e-3 * mx);
    sum = sum - (double)(P * P) * b0;
    double p[5] = {fmax(sum, mx), (double)(P / 2), (double)(P / 2), sigma0, b0};
#ifdef MIVIT_ML_STAGE_PATCH
    patch = stage;
#endif
    Fisher cur, nxt;
    int st = 2, it = 0;                                                   // iteration cap
    if (!finite) {
        st = 3;
        for (int k = 0; k < 5; ++k) p[k] = nan;
        cur.cost = nan;
        cur.mag = 0.0;
    } else {
        ml_eval(patch, P, cam, p, fs, tab, L, cur);
        if (cur.bad) st = 1;                                              // no photons at all: no point to start from
        else if (!(cur.cost < 1e300)) st = 3;
    }
    double lambda = 1e-3;
    for (; it < SF_MAX_ITER && st == 2; ++it) {
        double d[5];
        if (!ml_solve(cur, lambda, d)) {
            lambda = lambda * 10.0;
            if (lambda > 1e10) st = 1;
            continue;
        }
        // rg_kernel's stopping rule: the undamped step against each parameter's scale
        const double a0 = fabs(p[0]), a4 = fabs(p[4]);
        const double sc[5] = {a0, fmax(fabs(p[1]), 1.0), fmax(fabs(p[2]), 1.0), fabs(p[3]), fmax(a4, a0)};
        double d0[5];
        bool small = ml_solve(cur, 0.0, d0);
        for (int k = 0; k < 5; ++k) small = small && fabs(d0[k]) <= xtol * sc[k];
        double q[5];
        for (int k = 0; k < 5; ++k) q[k] = p[k] + d[k];
        ml_eval(patch, P, cam, q, fs, tab, L, nxt);
        // accepted unless the cost rises by more than its own rounding error, which for a deviance is relative to the magnitude
        // of the summed terms (csrc/spot_fit.h, "the slack")
        if (!nxt.bad && nxt.cost <= cur.cost + SF_COST_SLACK * cur.mag) {
            for (int k = 0; k < 5; ++k) p[k] = q[k];
            cur = nxt;
            lambda = fmax(lambda * 0.1, 1e-12);
        } else {
            lambda = lambda * 10.0;
            if (lambda > 1e10) st = 1;
        }
        if (small) st = 0;
    }
    double v[5];
    bool have = st == 0 && ml_crlb(cur, v);
    if (have && !fs) v[3] = 0.0;
    for (int k = 0; k < 5; ++k) {
        params[(int64_t)i * 5 + k] = p[k];
        crlb[(int64_t)i * 5 + k] = have ? v[k] : nan;
    }
    deviance[i] = cur.cost;
    status[i] = st;
    iterations[i] = it;
}

}  // namespace

extern "C" int mivit_fit_spots_mle(const float *patches, int N, int P, double gain, double offset, double read_var,
                                   double sigma0, int fit_sigma, double xtol, double *params, double *crlb, double *deviance,
                                   int *status, int *iterations, void *stream) {
    MIVIT_CHECK(N >= 0, "fit_spots_mle: N = %d < 0", N);
    if (sf_check_patch_fit("fit_spots_mle", P, xtol, &sigma0)) return 1;
    if (sf_check_camera("fit_spots_mle", gain, offset, read_var)) return 1;
    MIVIT_CHECK(fit_sigma == 0 || fit_sigma == 1, "fit_spots_mle: fit_sigma = %d (0 or 1)", fit_sigma);
    if (N == 0) return 0;
    MIVIT_CHECK(patches && params && crlb && deviance && status && iterations, "fit_spots_mle: null pointer");
    const int tpb = sf_lanes_per_workgroup(N);
    size_t lds = (size_t)6 * P * tpb * sizeof(double);                    // <= 46 080 bytes
#ifdef MIVIT_ML_STAGE_PATCH
    lds += (size_t)P * P * tpb * sizeof(float);
    MIVIT_CHECK(lds <= 65536, "fit_spots_mle: a staged-patch build holds patches up to side 11, got %d", P);
#endif
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(ml_kernel, dim3((N + tpb - 1) / tpb), dim3(tpb), lds, static_cast<hipStream_t>(stream), patches, N, P,
                       Camera{gain, offset, read_var}, sigma0, fit_sigma, xtol, params, crlb, deviance, status, iterations);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
