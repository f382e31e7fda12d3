// What the four spot fits share (tracking.hip::rg_kernel, localize.hip::ml_kernel, localize2.hip::ml2_kernel, detect.hip::
// lr_kernel): the camera's conversion of a pixel, the constants of a patch fit, the host checks of the common arguments, and,
// for ml2_kernel and lr_kernel, the Cholesky factor of a damped matrix on a packed lower triangle with the solve and the
// diagonal of the inverse on top of it and the damped Newton (Levenberg-Marquardt) loop itself.  rg_kernel and ml_kernel keep
// their own text of the factorisation and of the loop, the same operations in the same order: on the shared ones they measured
// about 1 % slower than before in every form tried.  The description of the loop below is the one for all four.
// Nothing here knows a model: evaluations, starting points, LDS layouts, the kernels' mappings and outputs are in the model's
// file.
//
// The arithmetic is fp64 in a fixed order that the restatements of helpers/tracking.py repeat, so nothing may be contracted
// into FMA: the pragma below holds for the rest of the translation unit, and ONLY TRANSLATION UNITS THAT WANT NO CONTRACTION
// MAY INCLUDE THIS FILE.
#pragma once
#pragma clang fp contract(off)

#include "common.h"

// each translation unit that includes this gets its own copy (anonymous namespace, as csrc/peaks.h)
namespace {

constexpr int SF_MAX_P = 15;                  // largest patch side
constexpr int SF_MAX_ITER = 100;
constexpr double SF_COST_SLACK = 1e-13;       // of what the cost's rounding error scales with (sf_damped_fit)
constexpr double SF_MIN_SIGMA = 0.2;
constexpr double SF_SQRT2 = 1.4142135623730951, SF_SQRT_2PI = 2.5066282746310002;

// ------------------------------------------------------------------------------------------------
// the photon-counting camera: d = max((adu - offset) / gain, 0) + read_var
// ------------------------------------------------------------------------------------------------
struct Camera {
    double gain, offset, read_var;
};

__device__ __forceinline__ double sf_data(float v, const Camera &c) {
    const double e = ((double)v - c.offset) / c.gain;
    return (e > 0.0 ? e : 0.0) + c.read_var;
}

// ------------------------------------------------------------------------------------------------
// NP x NP symmetric matrices as the lower triangle row by row: A[i (i + 1) / 2 + j], j <= i.  A and g may point to registers
// or to LDS; every loop is unrolled, so no index is a run-time one and L, z, X stay in registers.  The three are left to the
// inliner (it inlines them everywhere) and only the loop below is forced in: lr_kernel measured level with the code before
// in this form and up to 2 % slower with all four forced.
// ------------------------------------------------------------------------------------------------
// Cholesky factor of A + lambda diag(A); false if the matrix is not positive definite (or not finite).  It returns at the first
// pivot that fails.  Whoever gets false discards L, so stopping early and factoring on with a stand-in pivot are observably
// the same; stopping is the less work where lanes hold different patches (one lane per patch), and where a whole wave holds
// one patch (ml2_kernel) every lane factors the same numbers, takes the same exit, and the call lies between two barriers,
// never across one.
template <int NP>
__device__ bool sf_chol(const double *A, double lambda, double *L) {
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = A[i * (i + 1) / 2 + j];
            if (i == j) s = s + lambda * s;
#pragma unroll
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
template <int NP>
__device__ bool sf_solve(const double *A, const double *g, double lambda, double *d) {
    double L[NP * (NP + 1) / 2];
    if (!sf_chol<NP>(A, lambda, L)) return false;
    double z[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        double s = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i * (i + 1) / 2 + k] * z[k];
        z[i] = s / L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = NP - 1; i >= 0; --i) {
        double s = z[i];
#pragma unroll
        for (int k = i + 1; k < NP; ++k) s = s - L[k * (k + 1) / 2 + i] * d[k];
        d[i] = s / L[i * (i + 1) / 2 + i];
    }
    return true;
}

// diagonal of A^-1 = L^-T L^-1: column j of X = L^-1 by forward substitution, v[j] = sum_i X[i][j]^2 (i ascending)
template <int NP>
__device__ bool sf_crlb(const double *A, double *v) {
    double L[NP * (NP + 1) / 2];
    if (!sf_chol<NP>(A, 0.0, L)) return false;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        double X[NP];
        X[j] = 1.0 / L[j * (j + 1) / 2 + j];
        double acc = X[j] * X[j];
#pragma unroll
        for (int i = j + 1; i < NP; ++i) {
            double s = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) s = s - L[i * (i + 1) / 2 + k] * X[k];
            X[i] = s / L[i * (i + 1) / 2 + i];
            acc = acc + X[i] * X[i];
        }
        v[j] = acc;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// The damped Newton loop.  A Fit holds the evaluation (cost, gradient g, matrix A) of the current point p and room for one
// more, and supplies
//   const double *A(), *g()             the current point's matrix (packed lower triangle) and gradient
//   void scales(const double *p, double *sc)   the scale of each parameter for the stopping rule
//   bool step(const double *q)          evaluates q into the spare point; true if q is acceptable: inside the model's
//                                       domain, and its cost does not exceed the current one by more than the slack (below)
//   void accept()                       makes the spare point the current one
// Called with st = 2 (it ends as the iteration cap's status unless something else happens) or with the status a bad start
// already has, in which case nothing runs.  Status: 0 converged, 1 singular (lambda past 1e10), 2 iteration cap, 3 not finite.
//
// One iteration: solve with the damped matrix A + lambda diag(A); a matrix that does not factor costs the iteration, lambda
// grows tenfold and the next one tries again.  Then the undamped (Gauss-Newton) step from the same point: the model's own
// estimate of the distance to the optimum, "small" when it is below xtol relative to each parameter's scale.  The damped step
// would also shrink when lambda grows, far from the optimum, so it cannot be the one the stopping rule looks at.  Then the
// damped step is tried: accepted, lambda falls tenfold (floor 1e-12); rejected, it grows tenfold.  Only then does "small" end
// the loop with status 0, so the last step taken from a converged point is kept when it is acceptable.
//
// The slack: a step is accepted unless the cost rises by more than its own rounding error.  Close to the optimum a step
// changes the cost by less than that, and a strict test would stop the iteration at sqrt(eps) of the parameters.  What the
// error is relative to depends on the cost, which is why the test is the Fit's: a sum of squares (rg_kernel) errs relative to
// itself, cost (1 + SF_COST_SLACK).  A Poisson deviance is a sum of differences mu - d + d log(d / mu) of terms hundreds of
// times larger than itself, and its error is relative to those, cost + SF_COST_SLACK mag with mag = 2 sum(mu + d): measured
// against the cost alone, a converged patch with a small deviance (P = 3: 0.3) had its last steps (1e-11 of the parameters, a
// "rise" of 1e-13 of the cost, all rounding) rejected four times over, and the count depended on the last bit of log()
// (DESIGN 4o).
// ------------------------------------------------------------------------------------------------
template <int NP, class Fit>
__device__ __forceinline__ void sf_damped_fit(Fit &fit, double *p, double xtol, int &st, int &it) {
    double lambda = 1e-3;
    for (; it < SF_MAX_ITER && st == 2; ++it) {
        double d[NP];
        if (!sf_solve<NP>(fit.A(), fit.g(), lambda, d)) {
            lambda = lambda * 10.0;
            if (lambda > 1e10) st = 1;
            continue;
        }
        double sc[NP];
        fit.scales(p, sc);
        double d0[NP];
        bool small = sf_solve<NP>(fit.A(), fit.g(), 0.0, d0);
#pragma unroll
        for (int k = 0; k < NP; ++k) small = small && fabs(d0[k]) <= xtol * sc[k];
        double q[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) q[k] = p[k] + d[k];
        if (fit.step(q)) {
#pragma unroll
            for (int k = 0; k < NP; ++k) p[k] = q[k];
            fit.accept();
            lambda = fmax(lambda * 0.1, 1e-12);
        } else {
            lambda = lambda * 10.0;
            if (lambda > 1e10) st = 1;
        }
        if (small) st = 0;
    }
}

// ------------------------------------------------------------------------------------------------
// host: the checks of the arguments the entry points share, and the launch shape of the one-lane-per-patch kernels
// ------------------------------------------------------------------------------------------------
inline int sf_check_camera(const char *name, double gain, double offset, double read_var) {
    MIVIT_CHECK(gain > 0.0 && gain < 1e300, "%s: gain = %g (need a finite gain > 0)", name, gain);
    MIVIT_CHECK(offset - offset == 0.0, "%s: offset = %g is not finite", name, offset);
    MIVIT_CHECK(read_var >= 0.0 && read_var < 1e300, "%s: read_var = %g (need a finite read_var >= 0)", name, read_var);
    return 0;
}

// sigma0: null for a fit that takes no starting width
inline int sf_check_patch_fit(const char *name, int P, double xtol, const double *sigma0) {
    MIVIT_CHECK(P >= 3 && P <= SF_MAX_P && (P & 1), "%s: patch side %d (odd, 3 .. %d)", name, P, SF_MAX_P);
    MIVIT_CHECK(!sigma0 || (*sigma0 > SF_MIN_SIGMA && *sigma0 < (double)P), "%s: sigma0 = %g (need %g < sigma0 < P = %d)", name,
                sigma0 ? *sigma0 : 0.0, SF_MIN_SIGMA, P);
    MIVIT_CHECK(xtol > 0.0 && xtol <= 1.49012e-8, "%s: xtol = %g (0 < xtol <= 1.49012e-8, MINPACK's default)", name, xtol);
    return 0;
}

// lanes per workgroup of a one-lane-per-patch launch: reach every CU (256) before filling waves
inline int sf_lanes_per_workgroup(int N) {
    int tpb = 64;
    while (tpb > 1 && (int64_t)tpb * 256 > N) tpb >>= 1;
    return tpb;
}

}  // namespace
