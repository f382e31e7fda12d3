// Likelihood-ratio particle detection on the photon-counting camera: per pixel, H0 "local background only" against
// H1 "background plus one PSF-shaped spot centred on this pixel", thresholded at a false-alarm probability (Serge et al., Nat.
// Methods 5, 687 (2008); Smith et al., Nat. Methods 12, 717 (2015)).  It stands beside the difference-of-Gaussians rule of
// csrc/tracking.hip, whose threshold is a fraction of the frame's own maximum, and shares its peak selection (csrc/peaks.h).
//
// Data d = max((adu - offset) / gain, 0) + read_var (csrc/spot_fit.h::sf_data).  Template g(dy, dx) = e[dy] e[dx] with e the
// pixel-integrated Gaussian centred on a pixel centre, 2 r + 1 values computed by the caller on the host.  The window of a
// pixel is the in-frame pixels with |dy|, |dx| <= r: clipped at the frame edge, not reflected.
//
// mivit_score_peaks, four launches whatever the frame count:
//   1. tk_init_kernel   (peaks.h)
//   2. sc_map_kernel    one workgroup per 16 x 64 tile.  The tile and a halo of r pixels go to LDS once as d in fp64, pixels
//                       outside the frame as 0: a clipped sum and a sum over the zero-padded window are the same bits, every
//                       term outside being + 0.0 added to a sum that starts at + 0.0.  Column pass from LDS into LDS
//                       (A = sum e[dy] d, B = sum d over ascending dy), row pass from that (Sgd = sum e[dx] A, Sd = sum B over
//                       ascending dx).  The window's own sums factor per axis: the count, sum e and sum e^2 of the valid
//                       offsets of each of the tile's 16 rows and 64 columns are six small LDS tables.  Then
//                       mu0 = Sd / n, U = Sgd - mu0 Sg, V = mu0 (Sgg - Sg Sg / n), S = U > 0 && V > 0 ? U U / V : 0,
//                       the score (Rao) statistic of theta = 0 in mu = theta g + beta; S to fp32, stored, reduced to the
//                       frame's max / min keys as tk_dog_kernel does.  No transcendental function, no atomics on the map.
//   3. tk_mask_kernel   (peaks.h) with the absolute threshold
//   4. tk_select_kernel (peaks.h)
//
// mivit_lrt_peaks: the exact Poisson likelihood ratio at every candidate of stage 1.  One wave per frame, one lane per
// candidate, 64 candidates at a time in stage-1 order: the fit is a short serial damped Newton loop on two parameters over at
// most 15 x 15 pixels (csrc/spot_fit.h::sf_damped_fit with ml_kernel's slack of the summed magnitudes), so a lane owns every
// sum and no order has to be pinned across lanes;
// the wave's ballot of "T > t" gives each kept candidate its slot, so a frame's survivors are compacted in stage-1 order
// without a second kernel or a read-back.  A movie has many frames, which is what fills the device; a frame has a few dozen
// candidates, which half-fill one wave.  The window is read from the movie in every evaluation (it is in L2 after stage 1); the
// profile is in LDS, because a lane indexes it by its own offset.
//
// No contraction into FMA: the score map agrees bitwise with helpers/tracking._score_numpy, the fit differs by log alone.
#pragma clang fp contract(off)

#include "common.h"
#include "peaks.h"
#include "spot_fit.h"

namespace {

constexpr int SC_MAX_R = 7;
constexpr double LR_XTOL = 1e-11;             // helpers/tracking.FIT_XTOL

struct ScoreArgs {
    const float *movie;       // [F, H, W]
    float *map;               // [F, H, W]
    int *maxkey, *minkey;     // [F]
    int H, W, r, tiles_x, tiles_y;
    Camera cam;
    double e[2 * SC_MAX_R + 1];   // e[k + r] the profile at offset k
};

__global__ __launch_bounds__(256) void sc_map_kernel(const ScoreArgs a) {
    extern __shared__ double sc_lds[];
    __shared__ int smax, smin;
    const int H = a.H, W = a.W, R = a.r;
    const int LW = TK_TX + 2 * R, LH = TK_TY + 2 * R;
    double *in = sc_lds;                 // LH x LW, d
    double *tA = in + LH * LW;           // TK_TY x LW, column pass weighted by e
    double *tB = tA + TK_TY * LW;        // TK_TY x LW, column pass unweighted
    double *ax = tB + TK_TY * LW;        // per axis: count, sum e, sum e^2 of the valid offsets; rows first, then columns
    double *ny = ax, *gy = ny + TK_TY, *qy = gy + TK_TY, *nx = qy + TK_TY, *gx = nx + TK_TX, *qx = gx + TK_TX;
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
        const int y = y0 + ly - R, x = x0 + lx - R;
        in[t] = (y >= 0 && y < H && x >= 0 && x < W) ? sf_data(src[(int64_t)y * W + x], a.cam) : 0.0;
    }
    if (threadIdx.x < TK_TY + TK_TX) {
        const bool row = threadIdx.x < TK_TY;
        const int l = row ? threadIdx.x : threadIdx.x - TK_TY;
        const int c = row ? y0 + l : x0 + l, lim = row ? H : W;
        double n = 0.0, g = 0.0, q = 0.0;
        for (int k = -R; k <= R; ++k)
            if (c + k >= 0 && c + k < lim) {
                const double e = a.e[k + R];
                n = n + 1.0;
                g = g + e;
                q = q + e * e;
            }
        (row ? ny : nx)[l] = n;
        (row ? gy : gx)[l] = g;
        (row ? qy : qx)[l] = q;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < TK_TY * LW; t += blockDim.x) {          // axis 0, all LW columns (halo included)
        const int ly = t / LW, lx = t - ly * LW;
        const double *c = in + (ly + R) * LW + lx;
        double sa = 0.0, sb = 0.0;
        for (int k = -R; k <= R; ++k) {
            const double v = c[k * LW];
            sa = sa + a.e[k + R] * v;
            sb = sb + v;
        }
        tA[t] = sa;
        tB[t] = sb;
    }
    __syncthreads();
    int kmax = INT32_MIN, kmin = INT32_MAX;
    for (int t = threadIdx.x; t < TK_TY * TK_TX; t += blockDim.x) {       // axis 1
        const int ly = t / TK_TX, lx = t - ly * TK_TX;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        const double *cA = tA + ly * LW + lx + R, *cB = tB + ly * LW + lx + R;
        double Sgd = 0.0, Sd = 0.0;
        for (int k = -R; k <= R; ++k) {
            Sgd = Sgd + a.e[k + R] * cA[k];
            Sd = Sd + cB[k];
        }
        const double n = ny[ly] * nx[lx], Sg = gy[ly] * gx[lx], Sgg = qy[ly] * qx[lx];
        const double mu0 = Sd / n;
        const double U = Sgd - mu0 * Sg;
        const double V = mu0 * (Sgg - Sg * Sg / n);
        const float S = (U > 0.0 && V > 0.0) ? (float)(U * U / V) : 0.f;
        a.map[((int64_t)f * H + y) * W + x] = S;
        const int key = ordered_key(S);
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
// stage 2: mu_k = theta g_k + beta over the clipped window, row-major
// ------------------------------------------------------------------------------------------------------------------------
struct LrtArgs {
    const float *movie;       // [F, H, W]
    const int *count_in;      // [F]
    const int *coords_in;     // [F, cap, 2]
    const float *values_in;   // [F, cap]
    int *count;               // [F]
    int *coords;              // [F, cap, 2]
    double *stats;            // [F, cap, 4]
    int *status;              // [F, cap]
    int H, W, r, cap;
    Camera cam;
    double threshold;
    double e[2 * SC_MAX_R + 1];
};

struct Window {
    const float *frame;
    const double *e;          // LDS, e[k + r]
    int W, r, y, x, ya, yb, xa, xb;
};

struct LrEval {
    double cost;              // the deviance against the data
    double mag;               // 2 sum(mu + d)
    double g[2];              // sum (1 - d / mu) (g, 1)
    double A[3];              // sum (g, 1)(g, 1)^T / mu, lower triangle row by row
    bool bad;                 // theta <= 0 or a pixel with mu <= 0
};

__device__ void lr_eval(const Window &w, const Camera &cam, double theta, double beta, LrEval &n) {
    n.cost = n.mag = n.g[0] = n.g[1] = n.A[0] = n.A[1] = n.A[2] = 0.0;
    bool bad = !(theta > 0.0);
    for (int yy = w.ya; yy <= w.yb; ++yy) {
        const double ey = w.e[yy - w.y + w.r];
        for (int xx = w.xa; xx <= w.xb; ++xx) {
            const double g = ey * w.e[xx - w.x + w.r];
            const double d = sf_data(w.frame[(int64_t)yy * w.W + xx], cam);
            const double mu = theta * g + beta;
            bad = bad || !(mu > 0.0);
            const double rm = 1.0 / mu, r = d * rm;
            n.cost = n.cost + (d > 0.0 ? (mu - d) + d * log(r) : mu);
            n.mag = n.mag + (mu + d);
            const double wt = 1.0 - r;
            n.g[0] = n.g[0] + g * wt;
            n.g[1] = n.g[1] + wt;
            const double gr = g * rm;
            n.A[0] = n.A[0] + gr * g;
            n.A[1] = n.A[1] + rm * g;
            n.A[2] = n.A[2] + rm;
        }
    }
    n.cost = 2.0 * n.cost;
    n.mag = 2.0 * n.mag;
    n.bad = bad;
}

// the two-parameter fit p = (theta, beta) as sf_damped_fit sees it
struct LrFit {
    const Window &w;
    const Camera &cam;
    LrEval cur, nxt;
    __device__ const double *A() const { return cur.A; }
    __device__ const double *g() const { return cur.g; }
    // one scale for both: at a faint candidate theta is far below beta, and its own magnitude would ask for less than the
    // gradient's rounding error
    __device__ void scales(const double *p, double *sc) const { sc[0] = sc[1] = fmax(fabs(p[0]), fabs(p[1])); }
    __device__ bool step(const double *q) {
        lr_eval(w, cam, q[0], q[1], nxt);
        return !nxt.bad && nxt.cost <= cur.cost + SF_COST_SLACK * cur.mag;
    }
    __device__ void accept() { cur = nxt; }
};

// -> status; T, theta, beta of the last accepted point
__device__ int lr_fit(const Window &w, const Camera &cam, double &T, double &theta, double &beta) {
    double n = 0.0, Sd = 0.0, Sgd = 0.0, Sg = 0.0, Sgg = 0.0;
    for (int yy = w.ya; yy <= w.yb; ++yy) {
        const double ey = w.e[yy - w.y + w.r];
        for (int xx = w.xa; xx <= w.xb; ++xx) {
            const double g = ey * w.e[xx - w.x + w.r];
            const double d = sf_data(w.frame[(int64_t)yy * w.W + xx], cam);
            n = n + 1.0;
            Sd = Sd + d;
            Sgd = Sgd + g * d;
            Sg = Sg + g;
            Sgg = Sgg + g * g;
        }
    }
    const double mu0 = Sd / n;
    const double U = Sgd - mu0 * Sg;
    const double den = Sgg - Sg * Sg / n;
    T = 0.0;
    theta = 0.0;
    beta = mu0;
    if (!(U > 0.0) || !(den > 0.0) || !(mu0 > 0.0)) return 0;             // the maximum is at theta = 0: H0 itself
    // least-squares start; where it leaves the domain (a spot far brighter than its window's mean allows): a thousandth of
    // the mean as background and the photons that keep the window's total
    theta = U / den;
    beta = mu0 - theta * Sg / n;
    if (!(beta > 0.0)) {
        beta = 1e-3 * mu0;
        theta = (Sd - n * beta) / Sg;
    }
    LrFit fit{w, cam};
    lr_eval(w, cam, theta, beta, fit.cur);
    int st = fit.cur.bad ? 1 : 2, it = 0;
    double p[2] = {theta, beta};
    sf_damped_fit<2>(fit, p, LR_XTOL, st, it);
    theta = p[0];
    beta = p[1];
    if (fit.cur.bad) {
        theta = 0.0;
        beta = mu0;
        return st;
    }
    double s1 = 0.0, s2 = 0.0;
    for (int yy = w.ya; yy <= w.yb; ++yy) {
        const double ey = w.e[yy - w.y + w.r];
        for (int xx = w.xa; xx <= w.xb; ++xx) {
            const double g = ey * w.e[xx - w.x + w.r];
            const double d = sf_data(w.frame[(int64_t)yy * w.W + xx], cam);
            const double mu = theta * g + beta;
            s1 = s1 + (d > 0.0 ? d * log(mu / mu0) : 0.0);
            s2 = s2 + mu;
        }
    }
    const double t = 2.0 * s1 - 2.0 * (s2 - Sd);
    T = t > 0.0 ? t : 0.0;
    return st;
}

__global__ __launch_bounds__(64) void lr_kernel(const LrtArgs a) {
    __shared__ double es[2 * SC_MAX_R + 1];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (lane == 0)
        for (int k = 0; k <= 2 * a.r; ++k) es[k] = a.e[k];
    __syncthreads();
    const int H = a.H, W = a.W, cap = a.cap;
    int nin = a.count_in[f];
    nin = nin < 0 ? 0 : (nin > cap ? cap : nin);
    Window w;
    w.frame = a.movie + (int64_t)f * H * W;
    w.e = es;
    w.W = W;
    w.r = a.r;
    int nkept = 0;
    for (int base = 0; base < nin; base += 64) {                          // uniform trip count: the ballot sees whole waves
        const int i = base + lane;
        bool keep = false;
        double T = 0.0, theta = 0.0, beta = 0.0;
        int st = 0, y = 0, x = 0;
        if (i < nin) {
            y = a.coords_in[((int64_t)f * cap + i) * 2];
            x = a.coords_in[((int64_t)f * cap + i) * 2 + 1];
            if (y >= 0 && y < H && x >= 0 && x < W) {
                w.y = y;
                w.x = x;
                w.ya = y - a.r < 0 ? 0 : y - a.r;
                w.yb = y + a.r > H - 1 ? H - 1 : y + a.r;
                w.xa = x - a.r < 0 ? 0 : x - a.r;
                w.xb = x + a.r > W - 1 ? W - 1 : x + a.r;
                st = lr_fit(w, a.cam, T, theta, beta);
                keep = T > a.threshold;
            }
        }
        const unsigned long long votes = __ballot(keep);
        if (keep) {
            const int64_t o = (int64_t)f * cap + nkept + __popcll(votes & ((1ull << lane) - 1ull));
            a.coords[o * 2] = y;
            a.coords[o * 2 + 1] = x;
            a.stats[o * 4] = T;
            a.stats[o * 4 + 1] = theta;
            a.stats[o * 4 + 2] = beta - a.cam.read_var;
            a.stats[o * 4 + 3] = (double)a.values_in[(int64_t)f * cap + i];
            a.status[o] = st;
        }
        nkept += __popcll(votes);
    }
    if (lane == 0) a.count[f] = nkept;
}

const char *check_profile(const double *e, int r) {
    for (int k = 0; k <= 2 * r; ++k)
        if (!(e[k] > 0.0) || !(e[k] <= 1.0)) return "a profile value outside (0, 1]";
    return nullptr;
}

}  // namespace

extern "C" size_t mivit_score_peaks_workspace_bytes(int F, int H, int W, int cap, int store_map) {
    if (F <= 0 || H <= 0 || W <= 0 || cap <= 0) return 0;
    // max key, min key per frame | candidate keys | the score map when the caller does not want it back
    size_t b = ((size_t)2 * F * sizeof(int) + 15) / 16 * 16 + (size_t)F * cap * sizeof(unsigned long long);
    if (!store_map) b += (size_t)F * H * W * sizeof(float);
    return b;
}

#define SC_CHECK_CAMERA(name)                                                                                            \
    MIVIT_CHECK(e, name ": null profile");                                                                              \
    MIVIT_CHECK(r >= 1 && r <= SC_MAX_R, name ": radius %d (1 .. %d)", r, SC_MAX_R);                                    \
    MIVIT_CHECK(H > r && W > r, name ": frames of %d x %d are not larger than the radius %d", H, W, r);                 \
    MIVIT_CHECK((int64_t)H * W <= INT32_MAX, name ": frames of %d x %d pixels", H, W);                                  \
    if (sf_check_camera(name, gain, offset, read_var)) return 1;                                                        \
    MIVIT_CHECK(threshold >= 0 && threshold < 1e30f, name ": threshold = %g (need a finite threshold >= 0)",            \
                (double)threshold);                                                                                     \
    MIVIT_CHECK(cap >= 1 && cap <= TK_MAX_CAP, name ": capacity of %d peaks per frame (1 .. %d)", cap, TK_MAX_CAP);     \
    MIVIT_CHECK(check_profile(e, r) == nullptr, name ": %s", check_profile(e, r))

extern "C" int mivit_score_peaks(const float *movie, int F, int H, int W, const double *e, int r, double gain, double offset,
                                 double read_var, float threshold, int min_distance, int cap, int *count, int *n_candidates,
                                 int *coords, float *values, float *map, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    MIVIT_CHECK(F >= 0, "score_peaks: F = %d < 0", F);
    SC_CHECK_CAMERA("score_peaks");
    MIVIT_CHECK(min_distance >= 1 && min_distance <= TK_MAX_MIN_DISTANCE, "score_peaks: min_distance = %d (1 .. %d)",
                min_distance, TK_MAX_MIN_DISTANCE);
    ScoreArgs a{};
    a.H = H;
    a.W = W;
    a.r = r;
    a.tiles_x = (W + TK_TX - 1) / TK_TX;
    a.tiles_y = (H + TK_TY - 1) / TK_TY;
    a.cam = Camera{gain, offset, read_var};
    const int64_t tiles = (int64_t)F * a.tiles_x * a.tiles_y, total = (int64_t)F * H * W;
    MIVIT_CHECK(tiles <= INT32_MAX && (total + 255) / 256 <= INT32_MAX, "score_peaks: movie of %d x %d x %d is too large", F,
                H, W);
    for (int k = 0; k <= 2 * r; ++k) a.e[k] = e[k];
    if (F == 0) return 0;
    MIVIT_CHECK(movie && count && n_candidates && coords && values && workspace, "score_peaks: null pointer");
    const size_t need = mivit_score_peaks_workspace_bytes(F, H, W, cap, map != nullptr);
    MIVIT_CHECK(workspace_bytes >= need, "score_peaks: workspace of %zu bytes < %zu", workspace_bytes, need);
    char *ws = static_cast<char *>(workspace);
    a.maxkey = reinterpret_cast<int *>(ws);
    a.minkey = a.maxkey + F;
    ws += ((size_t)2 * F * sizeof(int) + 15) / 16 * 16;
    unsigned long long *cand = reinterpret_cast<unsigned long long *>(ws);
    ws += (size_t)F * cap * sizeof(unsigned long long);
    a.movie = movie;
    a.map = map ? map : reinterpret_cast<float *>(ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(tk_init_kernel, dim3((F + 255) / 256), dim3(256), 0, s, a.maxkey, a.minkey, n_candidates, F);
    MIVIT_LAUNCH_CHECK();
    const int LW = TK_TX + 2 * r, LH = TK_TY + 2 * r;
    const size_t lds = (size_t)(LH * LW + 2 * TK_TY * LW + 3 * (TK_TY + TK_TX)) * sizeof(double);   // <= 40 608 bytes
    hipLaunchKernelGGL(sc_map_kernel, dim3((unsigned)tiles), dim3(256), lds, s, a);
    MIVIT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tk_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.map, a.maxkey, a.minkey,
                       n_candidates, cand, total, H, W, min_distance, cap, threshold, 1);
    MIVIT_LAUNCH_CHECK();
    const int n2max = next_pow2(cap);
    hipLaunchKernelGGL(tk_select_kernel, dim3((unsigned)F), dim3(256),
                       (size_t)n2max * sizeof(unsigned long long) + (size_t)2 * cap * sizeof(int), s, cand, n_candidates, W,
                       min_distance, cap, n2max, count, coords, values);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_lrt_peaks(const float *movie, int F, int H, int W, const double *e, int r, double gain, double offset,
                               double read_var, double threshold, int cap, const int *count_in, const int *coords_in,
                               const float *values_in, int *count, int *coords, double *stats, int *status, void *stream) {
    MIVIT_CHECK(F >= 0, "lrt_peaks: F = %d < 0", F);
    SC_CHECK_CAMERA("lrt_peaks");
    LrtArgs a{};
    a.H = H;
    a.W = W;
    a.r = r;
    a.cap = cap;
    a.cam = Camera{gain, offset, read_var};
    a.threshold = threshold;
    for (int k = 0; k <= 2 * r; ++k) a.e[k] = e[k];
    if (F == 0) return 0;
    MIVIT_CHECK(movie && count_in && coords_in && values_in && count && coords && stats && status, "lrt_peaks: null pointer");
    MIVIT_CHECK(count != count_in && coords != coords_in, "lrt_peaks: the kept list must not alias the candidate list");
    a.movie = movie;
    a.count_in = count_in;
    a.coords_in = coords_in;
    a.values_in = values_in;
    a.count = count;
    a.coords = coords;
    a.stats = stats;
    a.status = status;
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(lr_kernel, dim3((unsigned)F), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
