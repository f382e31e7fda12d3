// Real-movie front end on the GPU: particle detection for a whole movie and the sub-pixel Gaussian fit of every localisation,
// the counterparts of the reference's per-frame Python in helpers/helpersTracking.py -- detect_particles (:12-57, two
// scipy.ndimage.gaussian_filter calls + skimage.feature.peak_local_max per frame) and the scipy.optimize.curve_fit inside
// add_refined_localization_to_dataframe (:555-604).  Linking is in csrc/linking.hip.
//
// mivit_dog_peaks, four launches whatever the frame count (kernels 1, 3 and 4 are in csrc/peaks.h, shared with csrc/detect.hip):
//   1. tk_init_kernel    per frame: max / min keys and the candidate counter.
//   2. tk_dog_kernel     one workgroup per 16 x 64 tile of a frame.  The tile and a halo of radius(sigma2) pixels (indices
//                        reflected as scipy's 'reflect' mode does, d c b a | a b c d | d c b a) go to LDS once; the axis-0 pass
//                        of both Gaussians is written back to LDS rounded to fp32 (scipy filters a float32 image axis by axis
//                        into a float32 array), the axis-1 pass reads it from there.  Sums in fp64 in correlate1d's symmetric
//                        order: centre term, then (x[-k] + x[+k]) * w[k] from the outermost tap inwards.  dog = g1 - g2 in
//                        fp32, stored, and reduced to the frame's max and min (ordered-integer atomics, one pair per tile).
//   3. tk_mask_kernel    one thread per pixel: above threshold_percentage * max (one fp32 product) and not exceeded by any
//                        pixel of its (2 min_distance + 1)^2 window (replicated borders add no new value, so the window is
//                        just clipped) -> appended to the frame's candidate list through its counter as a 64-bit key.  A frame
//                        with min == max (every pixel a window maximum) has no candidate.
//   4. tk_select_kernel  one workgroup per frame: bitonic sort of the keys in LDS, then the greedy spacing pass.  The key is
//                        (inverted ordered value, row-major index), so the sort alone defines the order (value descending, ties
//                        by index ascending) whatever order the atomics appended in.
// Why this shape: the filter is the only part that touches every pixel more than once (2 x 17 + 2 x 9 taps at the default
// sigmas), and the tile's LDS copy turns that into one global read per pixel; the mask rejects > 99 % of the pixels on the
// threshold test before it looks at a window; a frame has a few dozen candidates, so one workgroup sorts them in a few
// microseconds and the frames run side by side.
//
// mivit_refine_gaussian: one thread per patch (as csrc/features.hip does per trajectory).  A patch has at most 15 x 15 pixels
// and five parameters; the fit is a short serial Levenberg-Marquardt loop, and a movie yields thousands of patches, so the
// lanes are filled by patches rather than by pixels and no cross-lane reduction order has to be pinned.  The loop is the one
// csrc/spot_fit.h::sf_damped_fit describes, written out here with its own factorisation (rg_solve) because this kernel
// measured about 1 % slower on the shared templates: a change to the loop is made there, here and in ml_kernel.
//
// No contraction into FMA anywhere in this file: the filter agrees bitwise with the host restatement (helpers/tracking.py).
#pragma clang fp contract(off)

#include "common.h"
#include "peaks.h"
#include "spot_fit.h"

namespace {

constexpr int TK_MAX_RADIUS = 16;     // int(4 sigma + 0.5) of the wider Gaussian

// scipy 'reflect' (half-sample symmetric), one reflection; clamped so that rows / columns of a tile that lie outside the frame
// (their results are discarded) still read inside it
__device__ __forceinline__ int reflect_index(int i, int n) {
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

struct DogArgs {
    const float *movie;       // [F, H, W]
    float *dog;               // [F, H, W]
    int *maxkey, *minkey;     // [F]
    int H, W, r1, r2, tiles_x, tiles_y;
    double w1[TK_MAX_RADIUS + 1], w2[TK_MAX_RADIUS + 1];   // w[0] centre, w[k] weight at distance k
};

__global__ __launch_bounds__(256) void tk_dog_kernel(const DogArgs a) {
    extern __shared__ float tk_lds[];
    __shared__ int smax, smin;
    const int H = a.H, W = a.W, R = a.r2;
    const int LW = TK_TX + 2 * R, LH = TK_TY + 2 * R;
    float *in = tk_lds;                  // LH x LW
    float *t1 = in + LH * LW;            // TK_TY x LW, axis-0 pass of sigma1
    float *t2 = t1 + TK_TY * LW;         // TK_TY x LW, axis-0 pass of sigma2
    const int tpf = a.tiles_x * a.tiles_y;
    const int f = blockIdx.x / tpf, rem = blockIdx.x - f * tpf;
    const int ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
    const int y0 = ty * TK_TY, x0 = tx * TK_TX;
    const float *src = a.movie + (int64_t)f * H * W;
    if (threadIdx.x == 0) {
        smax = INT32_MIN;
        smin = INT32_MAX;
    }
    for (int t = threadIdx.x; t < LH * LW; t += blockDim.x) {
        const int ly = t / LW, lx = t - ly * LW;
        in[t] = src[(int64_t)reflect_index(y0 + ly - R, H) * W + reflect_index(x0 + lx - R, W)];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < TK_TY * LW; t += blockDim.x) {          // axis 0, all LW columns (halo included)
        const int ly = t / LW, lx = t - ly * LW;
        const float *c = in + (ly + R) * LW + lx;
        double a1 = (double)c[0] * a.w1[0];
        for (int k = a.r1; k >= 1; --k) a1 = a1 + ((double)c[-k * LW] + (double)c[k * LW]) * a.w1[k];
        double a2 = (double)c[0] * a.w2[0];
        for (int k = a.r2; k >= 1; --k) a2 = a2 + ((double)c[-k * LW] + (double)c[k * LW]) * a.w2[k];
        t1[t] = (float)a1;
        t2[t] = (float)a2;
    }
    __syncthreads();
    int kmax = INT32_MIN, kmin = INT32_MAX;
    for (int t = threadIdx.x; t < TK_TY * TK_TX; t += blockDim.x) {       // axis 1
        const int ly = t / TK_TX, lx = t - ly * TK_TX;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        const float *c1 = t1 + ly * LW + lx + R, *c2 = t2 + ly * LW + lx + R;
        double a1 = (double)c1[0] * a.w1[0];
        for (int k = a.r1; k >= 1; --k) a1 = a1 + ((double)c1[-k] + (double)c1[k]) * a.w1[k];
        double a2 = (double)c2[0] * a.w2[0];
        for (int k = a.r2; k >= 1; --k) a2 = a2 + ((double)c2[-k] + (double)c2[k]) * a.w2[k];
        float d = (float)a1 - (float)a2;
        if (d == 0.f) d = 0.f;                                            // -0 and +0 are one value for max and ties
        a.dog[((int64_t)f * H + y) * W + x] = d;
        const int key = ordered_key(d);
        kmax = key > kmax ? key : kmax;
        kmin = key < kmin ? key : kmin;
    }
    atomicMax(&smax, kmax);
    atomicMin(&smin, kmin);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(a.maxkey + f, smax);
        atomicMin(a.minkey + f, smin);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// five-parameter Gaussian fit, p = (amplitude, x0, y0, sigma, offset)
// ------------------------------------------------------------------------------------------------------------------------
struct Normal {
    double cost;              // sum of squared residuals
    double g[5];              // J^T r
    double A[15];             // J^T J, lower triangle row by row: A[i (i + 1) / 2 + j], j <= i
};

__device__ void rg_eval(const float *patch, int P, const double *p, Normal &n) {
    n.cost = 0.0;
    for (int i = 0; i < 5; ++i) n.g[i] = 0.0;
    for (int i = 0; i < 15; ++i) n.A[i] = 0.0;
    const double s2 = p[3] * p[3], s3 = s2 * p[3];
    for (int iy = 0; iy < P; ++iy)
        for (int ix = 0; ix < P; ++ix) {
            const double dx = (double)ix - p[1], dy = (double)iy - p[2];
            const double r2 = dx * dx + dy * dy;
            const double e = exp(-(r2 / (2.0 * s2)));
            const double ae = p[0] * e;
            const double r = (p[4] + ae) - (double)patch[iy * P + ix];
            const double J[5] = {e, ae * dx / s2, ae * dy / s2, ae * r2 / s3, 1.0};
            n.cost = n.cost + r * r;
            for (int i = 0; i < 5; ++i) {
                n.g[i] = n.g[i] + J[i] * r;
                for (int j = 0; j <= i; ++j) n.A[i * (i + 1) / 2 + j] = n.A[i * (i + 1) / 2 + j] + J[i] * J[j];
            }
        }
}

// solves (A + lambda diag(A)) d = -g by Cholesky; false if the matrix is not positive definite (or not finite)
__device__ bool rg_solve(const Normal &n, double lambda, double *d) {
    double L[15];
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

__global__ __launch_bounds__(64) void rg_kernel(const float *__restrict__ patches, int N, int P, double xtol, double *params,
                                                float *peak, int *status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float *patch = patches + (int64_t)i * P * P;
    float mx = patch[0], mn = patch[0];
    for (int t = 1; t < P * P; ++t) {
        const float v = patch[t];
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
    }
    // the reference's guess (patch.max(), P // 2, P // 2, 1.0, patch.min())
    double p[5] = {(double)mx, (double)(P / 2), (double)(P / 2), 1.0, (double)mn};
    Normal cur, nxt;
    rg_eval(patch, P, p, cur);
    double lambda = 1e-3;
    int st = 2;                                                           // iteration cap
    if (!(cur.cost < 1e300)) st = 3;                                      // not finite at the start
    for (int it = 0; it < SF_MAX_ITER && st == 2; ++it) {
        double d[5];
        if (!rg_solve(cur, lambda, d)) {
            lambda = lambda * 10.0;
            if (lambda > 1e10) st = 1;
            continue;
        }
        // converged when the undamped (Gauss-Newton) step, the model's own estimate of the distance to the optimum, is below
        // xtol relative to each parameter's scale (positions: pixels; offset: the intensity scale).  The damped step would
        // also shrink when lambda grows, far from the optimum.
        const double a0 = fabs(p[0]), a4 = fabs(p[4]);
        const double sc[5] = {a0, fmax(fabs(p[1]), 1.0), fmax(fabs(p[2]), 1.0), fabs(p[3]), fmax(a4, a0)};
        double d0[5];
        bool small = rg_solve(cur, 0.0, d0);
        for (int k = 0; k < 5; ++k) small = small && fabs(d0[k]) <= xtol * sc[k];
        double q[5];
        for (int k = 0; k < 5; ++k) q[k] = p[k] + d[k];
        rg_eval(patch, P, q, nxt);
        // accepted unless the cost rises by more than its own rounding error: close to the optimum a step changes the cost
        // by less than that, and a strict test would stop the iteration at sqrt(eps) of the parameters
        if (nxt.cost <= cur.cost * (1.0 + SF_COST_SLACK)) {
            for (int k = 0; k < 5; ++k) p[k] = q[k];
            cur = nxt;
            lambda = fmax(lambda * 0.1, 1e-12);
        } else {
            lambda = lambda * 10.0;
            if (lambda > 1e10) st = 1;
        }
        if (small) st = 0;
    }
    for (int k = 0; k < 5; ++k) params[(int64_t)i * 5 + k] = p[k];
    peak[i] = mx;
    status[i] = st;
}

}  // namespace

extern "C" size_t mivit_dog_peaks_workspace_bytes(int F, int H, int W, int cap, int store_dog) {
    if (F <= 0 || H <= 0 || W <= 0 || cap <= 0) return 0;
    // max key, min key per frame | candidate keys | the DoG movie when the caller does not want it back
    size_t b = ((size_t)2 * F * sizeof(int) + 15) / 16 * 16 + (size_t)F * cap * sizeof(unsigned long long);
    if (!store_dog) b += (size_t)F * H * W * sizeof(float);
    return b;
}

extern "C" int mivit_dog_peaks(const float *movie, int F, int H, int W, const double *w1, int r1, const double *w2, int r2,
                               float threshold_percentage, int min_distance, int cap, int *count, int *n_candidates,
                               int *coords, float *values, float *dog, void *workspace, size_t workspace_bytes,
                               void *stream) {
    MIVIT_CHECK(F >= 0, "dog_peaks: F = %d < 0", F);
    MIVIT_CHECK(w1 && w2, "dog_peaks: null weight array");
    MIVIT_CHECK(r1 >= 0 && r1 <= r2 && r2 <= TK_MAX_RADIUS, "dog_peaks: radii %d, %d (need 0 <= r1 <= r2 <= %d)", r1, r2,
                TK_MAX_RADIUS);
    MIVIT_CHECK(H > r2 && W > r2, "dog_peaks: frames of %d x %d are not larger than the filter radius %d", H, W, r2);
    MIVIT_CHECK((int64_t)H * W <= INT32_MAX, "dog_peaks: frames of %d x %d pixels", H, W);
    MIVIT_CHECK(min_distance >= 1 && min_distance <= TK_MAX_MIN_DISTANCE, "dog_peaks: min_distance = %d (1 .. %d)",
                min_distance, TK_MAX_MIN_DISTANCE);
    MIVIT_CHECK(cap >= 1 && cap <= TK_MAX_CAP, "dog_peaks: capacity of %d peaks per frame (1 .. %d)", cap, TK_MAX_CAP);
    MIVIT_CHECK(threshold_percentage == threshold_percentage, "dog_peaks: threshold_percentage is NaN");
    DogArgs a{};
    a.H = H;
    a.W = W;
    a.r1 = r1;
    a.r2 = r2;
    a.tiles_x = (W + TK_TX - 1) / TK_TX;
    a.tiles_y = (H + TK_TY - 1) / TK_TY;
    const int64_t tiles = (int64_t)F * a.tiles_x * a.tiles_y, total = (int64_t)F * H * W;
    MIVIT_CHECK(tiles <= INT32_MAX && (total + 255) / 256 <= INT32_MAX, "dog_peaks: movie of %d x %d x %d is too large", F, H,
                W);
    for (int k = 0; k <= r1; ++k) a.w1[k] = w1[k];
    for (int k = 0; k <= r2; ++k) a.w2[k] = w2[k];
    if (F == 0) return 0;
    MIVIT_CHECK(movie && count && n_candidates && coords && values && workspace, "dog_peaks: null pointer");
    const size_t need = mivit_dog_peaks_workspace_bytes(F, H, W, cap, dog != nullptr);
    MIVIT_CHECK(workspace_bytes >= need, "dog_peaks: workspace of %zu bytes < %zu", workspace_bytes, need);
    char *ws = static_cast<char *>(workspace);
    a.maxkey = reinterpret_cast<int *>(ws);
    a.minkey = a.maxkey + F;
    ws += ((size_t)2 * F * sizeof(int) + 15) / 16 * 16;
    unsigned long long *cand = reinterpret_cast<unsigned long long *>(ws);
    ws += (size_t)F * cap * sizeof(unsigned long long);
    a.movie = movie;
    a.dog = dog ? dog : reinterpret_cast<float *>(ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(tk_init_kernel, dim3((F + 255) / 256), dim3(256), 0, s, a.maxkey, a.minkey, n_candidates, F);
    MIVIT_LAUNCH_CHECK();
    const int LW = TK_TX + 2 * r2, LH = TK_TY + 2 * r2;
    const size_t lds = (size_t)(LH * LW + 2 * TK_TY * LW) * sizeof(float);
    hipLaunchKernelGGL(tk_dog_kernel, dim3((unsigned)tiles), dim3(256), lds, s, a);
    MIVIT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tk_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.dog, a.maxkey, a.minkey,
                       n_candidates, cand, total, H, W, min_distance, cap, threshold_percentage, 0);
    MIVIT_LAUNCH_CHECK();
    const int n2max = next_pow2(cap);
    hipLaunchKernelGGL(tk_select_kernel, dim3((unsigned)F), dim3(256),
                       (size_t)n2max * sizeof(unsigned long long) + (size_t)2 * cap * sizeof(int), s, cand, n_candidates, W,
                       min_distance, cap, n2max, count, coords, values);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_refine_gaussian(const float *patches, int N, int P, double xtol, double *params, float *peak,
                                     int *status, void *stream) {
    MIVIT_CHECK(N >= 0, "refine_gaussian: N = %d < 0", N);
    if (sf_check_patch_fit("refine_gaussian", P, xtol, nullptr)) return 1;
    if (N == 0) return 0;
    MIVIT_CHECK(patches && params && peak && status, "refine_gaussian: null pointer");
    const int tpb = sf_lanes_per_workgroup(N);
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(rg_kernel, dim3((N + tpb - 1) / tpb), dim3(tpb), 0, static_cast<hipStream_t>(stream), patches, N, P,
                       xtol, params, peak, status);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
