// Richardson-Lucy deconvolution with total-variation regularisation (RL-TV) and the mild Gaussian filter of the Denoising
// experiment: the GPU counterparts of the reference's per-frame Python loops apply_rl_tv_tensor_iter_list ->
// richardson_lucy_tv_iter_list (helpers/helpersGeneration.py:542-632, two scipy.signal.fftconvolve calls + tv_gradient per
// iteration) and of ski.filters.gaussian(frame, sigma=0.5) (:530).
//
// RL-TV: one workgroup per frame, every array of the frame in LDS.  The estimate (fp32) and the relative blur (fp64) carry a
// zero halo of K-1 pixels, so fftconvolve(..., mode='same') becomes a direct sum without bounds checks:
//     full[n][m] = sum_{a,b} k[a][b] x[n-a][m-b],   same[i][j] = full[i + (K-1)/2][j + (K-1)/2]
//     => same[i][j] = sum_{a,b} k[a][b] xp[i + K-1-a][j + K-1-b]    (xp: x shifted by K-1-(K-1)/2 into the halo)
// The taps are summed in row-major (a, b) order from 0.0 with a separate multiply and add, every other step in the reference's
// own precision (fp64 convolutions and division, fp32 estimate and TV gradient), so the kernel agrees bitwise with the host
// restatement in helpers/generation.py.  The reference's FFTs differ from any direct sum by ~1e-16 relative; that is the only
// difference to the reference (tests/test_denoise.py measures it).
//
// No contraction into FMA anywhere in this file, and the default IEEE division / sqrt (no fast-math flags in build.py).
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int RL_MAX_HW = 32;       // frame side
constexpr int RL_MAX_K = 15;        // PSF side
constexpr int RL_MAX_SNAP = 16;
constexpr int GF_MAX_RADIUS = 15;

struct RLArgs {
    const float *in;          // [B, S, H, W]
    const double *psf;        // [K, K]
    float *out;               // [B, n_snap, S, H, W]
    int64_t frame0;           // first frame (b * S + s) of this launch
    int S, H, W, K, n_snap;
    float tv_weight;
    int snap[RL_MAX_SNAP];    // strictly increasing 0-based iteration indices
};

__device__ __forceinline__ float clip_lo(float x, float lo) { return (x != x) ? x : (x > lo ? x : lo); }
__device__ __forceinline__ float clip_hi(float x, float hi) { return (x != x) ? x : (x < hi ? x : hi); }

__global__ __launch_bounds__(256) void rl_tv_kernel(const RLArgs a) {
    extern __shared__ double lds[];
    const int H = a.H, W = a.W, K = a.K, HW = H * W;
    const int Hp = H + K - 1, Wp = W + K - 1, halo = K - 1 - (K - 1) / 2;
    double *psf = lds;                                   // K*K
    double *relp = psf + K * K;                          // Hp*Wp, zero halo
    float *estp = reinterpret_cast<float *>(relp + Hp * Wp);   // Hp*Wp, zero halo
    float *img = estp + Hp * Wp;                         // HW, clipped input
    float *dxn = img + HW;                               // HW
    float *dyn = dxn + HW;                               // HW
    const int64_t f = a.frame0 + blockIdx.x;
    const int64_t b = f / a.S, s = f - b * a.S;
    const float *src = a.in + f * HW;

    for (int t = threadIdx.x; t < K * K; t += blockDim.x) psf[t] = a.psf[t];
    for (int t = threadIdx.x; t < Hp * Wp; t += blockDim.x) {
        relp[t] = 0.0;
        estp[t] = 0.f;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
        const int i = p / W, j = p - i * W;
        img[p] = clip_lo(src[p], 1e-6f);                 // np.clip(image, 1e-6, None) on the float32 frame
        estp[(i + halo) * Wp + j + halo] = 0.5f;
    }
    __syncthreads();

    const int n_iter = a.snap[a.n_snap - 1] + 1;
    int next = 0;
    for (int it = 0; it < n_iter; ++it) {
        // relative_blur = image / (fftconvolve(estimate, psf, 'same') + 1e-6)          (fp64)
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int i = p / W, j = p - i * W;
            double acc = 0.0;
            for (int ka = 0; ka < K; ++ka) {
                const float *row = estp + (i + K - 1 - ka) * Wp + j + K - 1;
                const double *kr = psf + ka * K;
                for (int kb = 0; kb < K; ++kb) acc = acc + kr[kb] * (double)row[-kb];
            }
            relp[(i + halo) * Wp + j + halo] = (double)img[p] / (acc + 1e-6);
        }
        __syncthreads();
        // estimate *= fftconvolve(relative_blur, psf[::-1, ::-1], 'same')            (product in fp64, stored fp32)
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int i = p / W, j = p - i * W;
            double acc = 0.0;
            for (int ka = 0; ka < K; ++ka) {
                const double *row = relp + (i + K - 1 - ka) * Wp + j + K - 1;
                const double *kr = psf + (K - 1 - ka) * K + K - 1;       // mirrored row K-1-ka, read backwards
                for (int kb = 0; kb < K; ++kb) acc = acc + kr[-kb] * row[-kb];
            }
            float *e = estp + (i + halo) * Wp + j + halo;
            *e = (float)((double)*e * acc);
        }
        __syncthreads();
        // tv_gradient, fp32: forward differences (0 in the last column / row), normalised by sqrt(dx^2 + dy^2 + 1e-8)
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int i = p / W, j = p - i * W;
            const float *e = estp + (i + halo) * Wp + j + halo;
            const float dx = j + 1 < W ? e[1] - e[0] : 0.f;
            const float dy = i + 1 < H ? e[Wp] - e[0] : 0.f;
            const float mag = sqrtf((dx * dx + dy * dy) + 1e-8f);
            dxn[p] = dx / mag;
            dyn[p] = dy / mag;
        }
        __syncthreads();
        // estimate -= tv_weight * grad; clip to [0, 1]
        const bool snap = it == a.snap[next];
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int i = p / W, j = p - i * W;
            float g = 0.f;
            if (j + 1 < W) g = g - dxn[p];
            if (j > 0) g = g + dxn[p - 1];
            if (i + 1 < H) g = g - dyn[p];
            if (i > 0) g = g + dyn[p - W];
            float *e = estp + (i + halo) * Wp + j + halo;
            const float v = clip_hi(clip_lo(*e - a.tv_weight * g, 0.f), 1.f);
            *e = v;
            if (snap) a.out[((b * a.n_snap + next) * a.S + s) * HW + p] = v;
        }
        if (snap) ++next;
        __syncthreads();
    }
}

struct GaussArgs {
    const float *in;          // [N, H, W]
    float *out;               // [N, H, W]
    int64_t frame0;
    int H, W, radius;
    double w[GF_MAX_RADIUS + 1];   // w[0] centre, w[k] = weight at distance k
};

// scipy.ndimage.correlate1d with a symmetric kernel, mode 'nearest': out = x[0] w[0] + sum_{k = r..1} (x[-k] + x[+k]) w[k]
__global__ __launch_bounds__(256) void gaussian_filter_kernel(const GaussArgs a) {
    extern __shared__ double lds[];
    const int H = a.H, W = a.W, HW = H * W, r = a.radius;
    double *x = lds, *t0 = lds + HW;
    const int64_t f = a.frame0 + blockIdx.x;
    for (int p = threadIdx.x; p < HW; p += blockDim.x) x[p] = (double)a.in[f * HW + p];
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {           // axis 0
        const int i = p / W, j = p - i * W;
        double acc = x[p] * a.w[0];
        for (int k = r; k >= 1; --k) {
            const int lo = i - k < 0 ? 0 : i - k, hi = i + k > H - 1 ? H - 1 : i + k;
            acc = acc + (x[lo * W + j] + x[hi * W + j]) * a.w[k];
        }
        t0[p] = acc;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {           // axis 1
        const int i = p / W, j = p - i * W;
        const double *row = t0 + i * W;
        double acc = row[j] * a.w[0];
        for (int k = r; k >= 1; --k) {
            const int lo = j - k < 0 ? 0 : j - k, hi = j + k > W - 1 ? W - 1 : j + k;
            acc = acc + (row[lo] + row[hi]) * a.w[k];
        }
        a.out[f * HW + p] = (float)acc;
    }
}

int threads_for(int HW) {
    int t = (HW + 63) / 64 * 64;
    return t > 256 ? 256 : t;
}

constexpr int64_t FRAMES_PER_LAUNCH = 1 << 24;

}  // namespace

extern "C" int mivit_rl_tv_deconvolve(const float *frames, int B, int S, int H, int W, const double *psf, int K,
                                      const int *snapshots, int n_snap, float tv_weight, float *out, void *stream) {
    MIVIT_CHECK(B >= 0 && S >= 0, "rl_tv_deconvolve: B = %d, S = %d", B, S);
    MIVIT_CHECK(H >= 1 && H <= RL_MAX_HW && W >= 1 && W <= RL_MAX_HW, "rl_tv_deconvolve: frames of %d x %d (1 .. %d)", H, W,
                RL_MAX_HW);
    MIVIT_CHECK(K >= 1 && K <= RL_MAX_K, "rl_tv_deconvolve: PSF of side %d (1 .. %d)", K, RL_MAX_K);
    MIVIT_CHECK(snapshots && n_snap >= 1 && n_snap <= RL_MAX_SNAP, "rl_tv_deconvolve: %d snapshots (1 .. %d)", n_snap,
                RL_MAX_SNAP);
    RLArgs a{};
    for (int k = 0; k < n_snap; ++k) {
        MIVIT_CHECK(snapshots[k] >= 0 && (k == 0 || snapshots[k] > snapshots[k - 1]),
                    "rl_tv_deconvolve: snapshot list must be non-negative and strictly increasing (entry %d = %d)", k,
                    snapshots[k]);
        a.snap[k] = snapshots[k];
    }
    const int64_t nf = (int64_t)B * S;
    if (nf == 0) return 0;
    MIVIT_CHECK(frames && psf && out, "rl_tv_deconvolve: null pointer");
    a.in = frames;
    a.psf = psf;
    a.out = out;
    a.S = S;
    a.H = H;
    a.W = W;
    a.K = K;
    a.n_snap = n_snap;
    a.tv_weight = tv_weight;
    const int Hp = H + K - 1, Wp = W + K - 1;
    const size_t lds = (size_t)(K * K + Hp * Wp) * sizeof(double) + (size_t)(Hp * Wp + 3 * H * W) * sizeof(float);
    prof_set_tag(MIVIT_PROF_OP);
    for (int64_t f0 = 0; f0 < nf; f0 += FRAMES_PER_LAUNCH) {
        a.frame0 = f0;
        const int64_t n = nf - f0 < FRAMES_PER_LAUNCH ? nf - f0 : FRAMES_PER_LAUNCH;
        hipLaunchKernelGGL(rl_tv_kernel, dim3((unsigned)n), dim3(threads_for(H * W)), lds, static_cast<hipStream_t>(stream),
                           a);
        MIVIT_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mivit_gaussian_filter_frames(const float *in, int N, int H, int W, double sigma, double truncate, float *out,
                                            void *stream) {
    MIVIT_CHECK(N >= 0, "gaussian_filter_frames: N = %d < 0", N);
    MIVIT_CHECK(H >= 1 && H <= RL_MAX_HW && W >= 1 && W <= RL_MAX_HW, "gaussian_filter_frames: frames of %d x %d (1 .. %d)",
                H, W, RL_MAX_HW);
    MIVIT_CHECK(sigma > 0.0 && truncate >= 0.0, "gaussian_filter_frames: sigma = %g, truncate = %g", sigma, truncate);
    const double rr = truncate * sigma + 0.5;
    MIVIT_CHECK(rr < GF_MAX_RADIUS + 1, "gaussian_filter_frames: radius int(%g * %g + 0.5) > %d", truncate, sigma,
                GF_MAX_RADIUS);
    GaussArgs a{};
    a.radius = (int)rr;
    // scipy.ndimage._filters._gaussian_kernel1d: phi(x) = exp(-0.5 / sigma^2 * x^2), x = -r .. r, divided by its sum (numpy's
    // pairwise summation: 8 partial sums once there are 8 or more terms)
    const int n = 2 * a.radius + 1;
    double phi[2 * GF_MAX_RADIUS + 1];
    const double c = -0.5 / (sigma * sigma);
    for (int k = 0; k < n; ++k) {
        const double x = (double)(k - a.radius);
        phi[k] = exp(c * (x * x));
    }
    double sum = 0.0;
    if (n < 8) {
        for (int k = 0; k < n; ++k) sum += phi[k];
    } else {
        double r8[8];
        for (int q = 0; q < 8; ++q) r8[q] = phi[q];
        int k = 8;
        for (; k + 8 <= n; k += 8)
            for (int q = 0; q < 8; ++q) r8[q] += phi[k + q];
        sum = ((r8[0] + r8[1]) + (r8[2] + r8[3])) + ((r8[4] + r8[5]) + (r8[6] + r8[7]));
        for (; k < n; ++k) sum += phi[k];
    }
    for (int k = 0; k <= a.radius; ++k) a.w[k] = phi[a.radius + k] / sum;
    if (N == 0) return 0;
    MIVIT_CHECK(in && out, "gaussian_filter_frames: null pointer");
    a.in = in;
    a.out = out;
    a.H = H;
    a.W = W;
    const size_t lds = (size_t)2 * H * W * sizeof(double);
    prof_set_tag(MIVIT_PROF_OP);
    for (int64_t f0 = 0; f0 < N; f0 += FRAMES_PER_LAUNCH) {
        a.frame0 = f0;
        const int64_t nb = N - f0 < FRAMES_PER_LAUNCH ? N - f0 : FRAMES_PER_LAUNCH;
        hipLaunchKernelGGL(gaussian_filter_kernel, dim3((unsigned)nb), dim3(threads_for(H * W)), lds,
                           static_cast<hipStream_t>(stream), a);
        MIVIT_LAUNCH_CHECK();
    }
    return 0;
}
