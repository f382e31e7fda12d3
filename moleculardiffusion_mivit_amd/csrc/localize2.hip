// Joint Poisson maximum-likelihood fit of a localisation and its nearest same-frame neighbour, with a Cramer-Rao bound per
// parameter, and the neighbour search that feeds it.  The single-emitter fit it stands beside is csrc/localize.hip::ml_kernel;
// the damped loop (lambda schedule, stopping rule on the undamped step, status codes, the cost slack 1e-13 taken of
// 2 sum(mu + d)) is csrc/spot_fit.h::sf_damped_fit for both; the Fisher information as the matrix, the bound through the
// Cholesky factor of the undamped matrix at the returned point, fit_sigma = 0 by zero dE/ds and a 1 on the diagonal are that
// one's.
//
// Model of a patch [P, P] with pixel centres at integers, p = (N1, x1, y1, N2, x2, y2, s, b), k = count in {1, 2} emitters:
//   mu(iy, ix) = b + sum_{e < k} N_e E(ix; x_e, s) E(iy; y_e, s) + read_var,   E as in csrc/localize.hip
// Data d = max((patch - offset) / gain, 0) + read_var.  count = 1 is the five-parameter fit by the device of fit_sigma = 0:
// the derivatives of emitter 2 are zero, its diagonal entries are 1, so the eight-by-eight factor is the five-by-five one with
// rows of zeros added, term by term, and the steps of emitter 2 are exactly 0; its parameters and bounds are returned as NaN.
//
// Mapping: ONE WAVE PER PATCH (a workgroup is one wave).  One thread per patch, as in ml_kernel, does not carry over: matrix,
// factor and axis tables are indexed at run time, so they would have to live in LDS per lane, about 1.6 KB a lane at P = 9,
// which is one wave per CU.  A whole wave rather than a fraction of one, because then every branch of the damped loop is
// uniform by construction (every lane holds the same parameters and takes the same decisions), a barrier is never met in
// divergent code, and the three parallel phases fit a wave: 4 (P + 1) <= 64 pixel edges, 4 P <= 60 table entries, 46 sums.
// An evaluation is four phases with a barrier between them:
//   1. edges   lane l < 4 (P + 1): erf and exp at edge l % (P + 1) of axis l / (P + 1) (x1, y1, x2, y2)
//   2. tables  lane l < 4 P: E, dE/dc, dE/ds of pixel l % P of axis l / P from its two edges
//   3. pixels  lane l takes the pixels l, l + 64, ...: mu, 1 / mu, 1 - d / mu, the deviance term, mu + d and the eight
//              derivatives J of mu, each a function of that pixel alone, stored as [quantity][pixel]
//   4. sums    lane l < 46 OWNS one sum and adds its P^2 terms IN PIXEL ORDER (t = iy P + ix ascending): lanes 0 .. 35 the
//              lower triangle A[i (i + 1) / 2 + j] = sum (J_i / mu) J_j, lanes 36 .. 43 the gradient sum J_i (1 - d / mu), lane 44
//              the deviance, lane 45 sum (mu + d).  One loop serves all: sum (a[t] m[t]) b[t] with m = 1 - d / mu, b = J_7 = 1 for
//              the gradient and m = b = 1 for the last two; a product with 1.0 is exact.
// No sum crosses lanes, so no reduction order has to be pinned, there is no atomic, and a patch's bits depend on nothing but
// the patch: not on the batch, its position in it, or N.  The 8 x 8 factorisations and solves are done by every lane on the same
// numbers (registers, loops unrolled so that no index is a run-time one): it is the simplest place, and the lanes would
// otherwise idle.  LDS per wave: 8 (P + 1) + 12 P + 12 P^2 + 96 doubles = 24 832 bytes at P = 15, 10 048 at P = 9.
//
// No contraction into FMA: the host restatement (helpers/tracking._fit_mle2_numpy) differs by erf, exp and log alone.
#pragma clang fp contract(off)

#include "common.h"
#include "spot_fit.h"

namespace {

constexpr int M2_NP = 8;              // parameters
constexpr int M2_NA = 36;             // lower triangle
constexpr int M2_NSUM = 46;           // + 8 gradient entries + deviance + magnitude
constexpr int M2_SLOT = 48;           // doubles per set of sums in LDS
constexpr int M2_NQ = 12;             // per-pixel quantities: J_0 .. J_7, 1 / mu, 1 - d / mu, deviance term, mu + d
constexpr int M2_WAVE = 64;
constexpr int M2_MAX_GRID = 1 << 20;  // workgroups of a launch

__host__ __device__ constexpr int m2_lds_doubles(int P) { return 8 * (P + 1) + 12 * P + M2_NQ * P * P + 2 * M2_SLOT; }

// outside the model's domain: an N_e <= 0, s outside (0.2, P), a centre outside [-1, P]
__device__ __forceinline__ bool m2_outside(const double *p, int P, bool two) {
    bool bad = !(p[0] > 0.0) || !(p[6] > SF_MIN_SIGMA) || !(p[6] < (double)P);
    bad = bad || !(p[1] >= -1.0) || !(p[1] <= (double)P) || !(p[2] >= -1.0) || !(p[2] <= (double)P);
    if (two) bad = bad || !(p[3] > 0.0) || !(p[4] >= -1.0) || !(p[4] <= (double)P) || !(p[5] >= -1.0) || !(p[5] <= (double)P);
    return bad;
}

// The sums of one evaluation into out[0 .. 45] (LDS); returns "a pixel with mu <= 0".  Called by the whole wave in uniform
// control flow, p inside the domain.  sa, sm, sb: the three arrays of this lane's sum (phase 4 above), set once per patch.
__device__ bool m2_eval(const float *patch, int P, const Camera &cam, const double *p, bool two, bool fs, double *lds, double *out,
                        int lane, const double *sa, const double *sm, const double *sb) {
    const int PP = P * P, E1 = P + 1;
    double *edge_e = lds, *edge_g = lds + 4 * E1, *tab = lds + 8 * E1, *pix = tab + 12 * P;
    const double s = p[6];
    const double w = SF_SQRT2 * s, nc = 1.0 / (SF_SQRT_2PI * s), ns = nc / s;
    if (lane < 4 * E1) {
        const int a = lane / E1, k = lane - a * E1;
        const double c = a == 0 ? p[1] : a == 1 ? p[2] : a == 2 ? p[4] : p[5];
        const double t = ((double)k - 0.5) - c;
        const double u = t / w;
        edge_e[lane] = erf(u);
        edge_g[lane] = exp(-(u * u));
    }
    __syncthreads();
    if (lane < 4 * P) {
        const int a = lane / P, k = lane - a * P;
        const double c = a == 0 ? p[1] : a == 1 ? p[2] : a == 2 ? p[4] : p[5];
        const double t0 = ((double)k - 0.5) - c, t1 = ((double)(k + 1) - 0.5) - c;
        const double e0 = edge_e[a * E1 + k], e1 = edge_e[a * E1 + k + 1], g0 = edge_g[a * E1 + k], g1 = edge_g[a * E1 + k + 1];
        tab[(a * 3 + 0) * P + k] = 0.5 * (e1 - e0);
        tab[(a * 3 + 1) * P + k] = (g0 - g1) * nc;
        tab[(a * 3 + 2) * P + k] = fs ? (t0 * g0 - t1 * g1) * ns : 0.0;
    }
    __syncthreads();
    bool nonpos = false;
    const double *x1 = tab, *y1 = tab + 3 * P, *x2 = tab + 6 * P, *y2 = tab + 9 * P;
    for (int t = lane; t < PP; t += M2_WAVE) {
        const int iy = t / P, ix = t - iy * P;
        const double Ex1 = x1[ix], dEx1 = x1[P + ix], sEx1 = x1[2 * P + ix], Ey1 = y1[iy];
        const double nEy1 = p[0] * Ey1, ndEy1 = p[0] * y1[P + iy], nsEy1 = p[0] * y1[2 * P + iy];
        double mu = p[7] + nEy1 * Ex1;
        double J3 = 0.0, J4 = 0.0, J5 = 0.0, J6 = nEy1 * sEx1 + nsEy1 * Ex1;
        if (two) {
            const double Ex2 = x2[ix], dEx2 = x2[P + ix], sEx2 = x2[2 * P + ix], Ey2 = y2[iy];
            const double nEy2 = p[3] * Ey2, ndEy2 = p[3] * y2[P + iy], nsEy2 = p[3] * y2[2 * P + iy];
            mu = mu + nEy2 * Ex2;
            J3 = Ex2 * Ey2;
            J4 = nEy2 * dEx2;
            J5 = ndEy2 * Ex2;
            J6 = J6 + (nEy2 * sEx2 + nsEy2 * Ex2);
        }
        mu = mu + cam.read_var;
        nonpos = nonpos || !(mu > 0.0);
        const double d = sf_data(patch[t], cam);
        const double rm = 1.0 / mu, r = d * rm;
        pix[0 * PP + t] = Ex1 * Ey1;
        pix[1 * PP + t] = nEy1 * dEx1;
        pix[2 * PP + t] = ndEy1 * Ex1;
        pix[3 * PP + t] = J3;
        pix[4 * PP + t] = J4;
        pix[5 * PP + t] = J5;
        pix[6 * PP + t] = J6;
        pix[7 * PP + t] = 1.0;
        pix[8 * PP + t] = rm;
        pix[9 * PP + t] = 1.0 - r;
        pix[10 * PP + t] = d > 0.0 ? (mu - d) + d * log(r) : mu;
        pix[11 * PP + t] = mu + d;
    }
    __syncthreads();
    if (lane < M2_NSUM) {
        double acc = 0.0;
        for (int t = 0; t < PP; ++t) acc = acc + (sa[t] * sm[t]) * sb[t];      // pixel order
        if (lane >= M2_NA + M2_NP) acc = 2.0 * acc;                            // the deviance and its magnitude
        if (!fs && lane == 6 * 7 / 2 + 6) acc = 1.0;
        if (!two && (lane == 3 * 4 / 2 + 3 || lane == 4 * 5 / 2 + 4 || lane == 5 * 6 / 2 + 5)) acc = 1.0;
        out[lane] = acc;
    }
    const bool any = __any(nonpos) != 0;
    __syncthreads();
    return any;
}

// The joint fit as sf_damped_fit sees it.  The two sets of sums in LDS are the current point's and the spare one's: accepting
// flips which is which.  Every lane holds the same numbers, so the loop's branches are uniform and step's barriers are met
// by the whole wave.
struct M2Fit {
    const float *patch;
    int P;
    const Camera &cam;
    bool two, fs;
    double *lds, *sums;
    int lane;
    const double *sa, *sm, *sb;
    int c;                    // which set of sums is the current point's
    double cost, mag;         // the current point's
    __device__ const double *S() const { return sums + c * M2_SLOT; }
    __device__ const double *A() const { return S(); }
    __device__ const double *g() const { return S() + M2_NA; }
    // ml_kernel's scales, the photons of the brighter emitter for the background
    __device__ void scales(const double *p, double *sc) const {
        const double a0 = fmax(fabs(p[0]), fabs(p[3]));
        sc[0] = fabs(p[0]), sc[1] = fmax(fabs(p[1]), 1.0), sc[2] = fmax(fabs(p[2]), 1.0), sc[3] = fabs(p[3]);
        sc[4] = fmax(fabs(p[4]), 1.0), sc[5] = fmax(fabs(p[5]), 1.0), sc[6] = fabs(p[6]), sc[7] = fmax(fabs(p[7]), a0);
    }
    __device__ bool step(const double *q) {
        bool bad = m2_outside(q, P, two);
        double *T = sums + (1 - c) * M2_SLOT;
        if (!bad) bad = m2_eval(patch, P, cam, q, two, fs, lds, T, lane, sa, sm, sb);
        return !bad && T[44] <= cost + SF_COST_SLACK * mag;
    }
    __device__ void accept() {
        c = 1 - c;
        cost = S()[44];
        mag = S()[45];
    }
};

// the fit of patch i by the whole wave
__device__ void m2_patch(int64_t i, double *m2_lds, const float *__restrict__ patches, const int *__restrict__ count,
                         const double *__restrict__ guess, int P, const Camera &cam, double sigma0, int fit_sigma, double xtol,
                         double *params, double *crlb, double *deviance, int *status, int *iterations) {
    const int lane = threadIdx.x, PP = P * P;
    const bool fs = fit_sigma != 0;
    const float *patch = patches + i * PP;
    double *pix = m2_lds + 8 * (P + 1) + 12 * P, *sums = pix + M2_NQ * PP;
    // this lane's sum (m2_eval, phase 4)
    const double *sa = pix, *sm = pix + 7 * PP, *sb = pix + 7 * PP;
    if (lane < M2_NA) {
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= lane) ++r;
        sa = pix + r * PP;
        sm = pix + 8 * PP;
        sb = pix + (lane - r * (r + 1) / 2) * PP;
    } else if (lane < M2_NA + M2_NP) {
        sa = pix + (lane - M2_NA) * PP;
        sm = pix + 9 * PP;
    } else if (lane < M2_NSUM) {
        sa = pix + (10 + lane - (M2_NA + M2_NP)) * PP;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int cnt = count[i];
    const bool two = cnt == 2;
    // start, every lane on every pixel (the same address in all lanes: one request): background = the smallest pixel (at
    // least 1e-3 of the largest), photons = what lies above it, in pixel order, split evenly between the emitters
    bool finite = cnt == 1 || cnt == 2;
    double mx = sf_data(patch[0], cam), mn = mx, sum = 0.0;
    for (int t = 0; t < PP; ++t) {
        const float v = patch[t];
        finite = finite && (v - v == 0.f);
        const double d = sf_data(v, cam);
        mx = d > mx ? d : mx;
        mn = d < mn ? d : mn;
        sum = sum + d;
    }
    double g4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 4; ++k)
        if (k < 2 || two) {
            g4[k] = guess[i * 4 + k];
            finite = finite && (g4[k] - g4[k] == 0.0);
        }
    const double b0 = fmax(mn, 1e-3 * mx);
    sum = sum - (double)PP * b0;
    const double n0 = fmax(sum, mx);
    double p[M2_NP] = {two ? 0.5 * n0 : n0, g4[0], g4[1], two ? 0.5 * n0 : 0.0, g4[2], g4[3], sigma0, b0};
    M2Fit fit{patch, P, cam, two, fs, m2_lds, sums, lane, sa, sm, sb, 0, 0.0, 0.0};
    int st = 2, it = 0;                                                   // iteration cap
    if (!finite) {
        st = 3;
        for (int k = 0; k < M2_NP; ++k) p[k] = nan;
        fit.cost = nan;
    } else if (m2_outside(p, P, two) || (two && p[1] == p[4] && p[2] == p[5])) {
        // no photons at all, a guess outside the patch, or two guesses on one point: there the emitters are interchangeable, the
        // matrix is singular by symmetry and the gradient cannot tell them apart; only rounding would, differently on every
        // machine, so such a start ends as the singular matrix it is
        st = 1;
    } else {
        const bool bad = m2_eval(patch, P, cam, p, two, fs, m2_lds, sums, lane, sa, sm, sb);
        fit.cost = sums[44];
        fit.mag = sums[45];
        if (bad) st = 1;
        else if (!(fit.cost < 1e300)) st = 3;
    }
    sf_damped_fit<M2_NP>(fit, p, xtol, st, it);
    double v[M2_NP];
    const bool have = st == 0 && sf_crlb<M2_NP>(fit.A(), v);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < M2_NP; ++k) {
            const bool dead = !two && k >= 3 && k < 6;
            params[i * M2_NP + k] = dead ? nan : p[k];
            crlb[i * M2_NP + k] = !have || dead ? nan : (!fs && k == 6 ? 0.0 : v[k]);
        }
        deviance[i] = fit.cost;
        status[i] = st;
        iterations[i] = it;
    }
}

__global__ __launch_bounds__(M2_WAVE) void ml2_kernel(const float *__restrict__ patches, const int *__restrict__ count,
                                                      const double *__restrict__ guess, int N, int P, Camera cam, double sigma0,
                                                      int fit_sigma, double xtol, double *params, double *crlb, double *deviance,
                                                      int *status, int *iterations) {
    extern __shared__ double m2_lds[];                                    // m2_lds_doubles(P)
    // one wave per patch; a grid smaller than N (M2_MAX_GRID) walks the patches in strides.  The first barrier of a patch
    // is passed only when every lane has left the one before, so the LDS is free to be written again.
    for (int64_t i = blockIdx.x; i < N; i += gridDim.x)
        m2_patch(i, m2_lds, patches, count, guess, P, cam, sigma0, fit_sigma, xtol, params, crlb, deviance, status, iterations);
}

// One thread per row of the detections table, sorted by frame: the row scans the rows of its own frame in ascending index.
__global__ __launch_bounds__(256) void nb_kernel(const int *__restrict__ frame_offsets, const int *__restrict__ ys,
                                                 const int *__restrict__ xs, int F, int n, int reach, int *neighbour,
                                                 int *n_neighbours) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // the frame of row i: the last f with frame_offsets[f] <= i (fixed trip count whatever the offsets hold)
    int lo = 0, hi = F;                                                   // the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (frame_offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    int a = frame_offsets[lo], b = frame_offsets[lo + 1];
    a = a < 0 ? 0 : a;                                                    // no row outside the table is read
    b = b > n ? n : b;
    const int64_t y = ys[i], x = xs[i];
    int best = -1, within = 0;
    int64_t best_d2 = 0;
    for (int j = a; j < b; ++j) {
        if (j == i) continue;
        int64_t dy = (int64_t)ys[j] - y, dx = (int64_t)xs[j] - x;
        dy = dy < 0 ? -dy : dy;
        dx = dx < 0 ? -dx : dx;
        if (dy > reach || dx > reach) continue;
        ++within;
        const int64_t d2 = dy * dy + dx * dx;
        if (best < 0 || d2 < best_d2) {                                   // ties stay with the lower row index
            best = j;
            best_d2 = d2;
        }
    }
    neighbour[i] = best;
    n_neighbours[i] = within;
}

}  // namespace

extern "C" int mivit_fit_spots_mle2(const float *patches, const int *count, const double *guess, int N, int P, double gain,
                                    double offset, double read_var, double sigma0, int fit_sigma, double xtol, double *params,
                                    double *crlb, double *deviance, int *status, int *iterations, void *stream) {
    MIVIT_CHECK(N >= 0, "fit_spots_mle2: N = %d < 0", N);
    if (sf_check_patch_fit("fit_spots_mle2", P, xtol, &sigma0)) return 1;
    if (sf_check_camera("fit_spots_mle2", gain, offset, read_var)) return 1;
    MIVIT_CHECK(fit_sigma == 0 || fit_sigma == 1, "fit_spots_mle2: fit_sigma = %d (0 or 1)", fit_sigma);
    if (N == 0) return 0;
    MIVIT_CHECK(patches && count && guess && params && crlb && deviance && status && iterations, "fit_spots_mle2: null pointer");
    const size_t lds = (size_t)m2_lds_doubles(P) * sizeof(double);        // <= 24 832 bytes
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(ml2_kernel, dim3(N < M2_MAX_GRID ? N : M2_MAX_GRID), dim3(M2_WAVE), lds, static_cast<hipStream_t>(stream),
                       patches, count, guess, N, P,
                       Camera{gain, offset, read_var}, sigma0, fit_sigma, xtol, params, crlb, deviance, status, iterations);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_spot_neighbours(const int *frame_offsets, const int *ys, const int *xs, int F, int n, int reach,
                                     int *neighbour, int *n_neighbours, void *stream) {
    MIVIT_CHECK(F >= 0, "spot_neighbours: F = %d < 0", F);
    MIVIT_CHECK(n >= 0, "spot_neighbours: n = %d < 0", n);
    MIVIT_CHECK(reach >= 0, "spot_neighbours: reach = %d < 0", reach);
    if (n == 0) return 0;
    MIVIT_CHECK(F >= 1, "spot_neighbours: %d rows but no frame", n);
    MIVIT_CHECK(frame_offsets && ys && xs && neighbour && n_neighbours, "spot_neighbours: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(nb_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), frame_offsets, ys, xs, F,
                       n, reach, neighbour, n_neighbours);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
