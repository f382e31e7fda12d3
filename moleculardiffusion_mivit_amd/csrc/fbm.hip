// Fractional Gaussian noise: the increments of anomalous diffusion, MSD ~ t^alpha (the displacement law of the reference's
// disp_fbm, Experiments/mitochondria_simulation/mitochnodria.py:436-476, which takes them from the `fbm` package).  Exact:
// out = L z, L the lower Cholesky factor of the Toeplitz matrix of the autocovariance gamma, by the Durbin-Levinson (Hosking)
// recursion, which is algebraically that product, needs O(T) memory and keeps no factor in HBM.
//
// mivit_fgn, one launch: one workgroup of 256 threads per trajectory.  gamma's row, the prediction coefficients phi and the
// histories of the C axes (which share phi) live in LDS, (2 + C) T doubles; z is staged in the history buffer and g[n]
// overwrites z[n], so the loads and stores of global memory are two linear copies.  Step n takes all three of its sums on the
// coefficients of step n - 1,
//     A = sum_j phi[j] gamma[n-j],  B_c = sum_j phi[j] g_c[n-j],  R_c = sum_j phi[n-j] g_c[n-j],   j = 1 .. n-1,
// so there is ONE reduction per step: thread t owns the terms j = 1 + t, 1 + t + 256, ... in ascending order, a xor butterfly
// sums the 64 lanes of a wave (both operands of every add are the same in all lanes that get it, so every lane holds the same
// bits), the four wave sums go through LDS and every thread adds them as (w0 + w1) + (w2 + w3).  Then, redundantly in all
// threads, kappa = (gamma[n] - A) / v, v = v (1 - kappa^2); thread c writes g_c[n] = ((B_c - kappa R_c) + kappa g_c[0]) +
// sqrt(v) z_c[n]; and the pair (phi[j], phi[n-j]), j <= n / 2, is updated in place by the one thread that owns it.  Two
// barriers a step.  The lane mapping and the tree are the same for every launch and do not depend on N: no atomics, a
// trajectory's result is bitwise the same alone and in any batch.  gamma = (1, 0, 0, ...), alpha = 1, gives kappa = 0 and
// out = z.  helpers/generation._fgn_host restates the same formula in numpy; the two differ in the order of the sums only.
//
// No contraction into FMA, as in diffusion.hip.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int FGN_THREADS = 256;
constexpr int FGN_WAVES = FGN_THREADS / 64;
static_assert(FGN_WAVES == 4, "the cross-wave sum is written out for four waves");
constexpr int FGN_MAX_T = 2048;       // (2 + C) T doubles of LDS: 64 KiB at C = 2, 96 KiB at C = 4 (ops.FGN_MAX_T)
constexpr int FGN_MAX_C = 4;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__host__ __device__ constexpr size_t fgn_lds_doubles(int T, int C) { return (size_t)(2 + C) * T + FGN_WAVES * (1 + 2 * C); }

template <int C>
__global__ __launch_bounds__(FGN_THREADS) void fgn_kernel(const double *__restrict__ z, const double *__restrict__ gamma,
                                                          const int *__restrict__ gamma_row, int U, int T,
                                                          double *__restrict__ out) {
    constexpr int Q = 1 + 2 * C;                                          // sums of a step: A, B_c, R_c
    extern __shared__ double fgn_lds[];
    double *gam = fgn_lds;                                                // [T]
    double *phi = gam + T;                                                // [T], entries 1 .. n
    double *g = phi + T;                                                  // [T][C]: g below the current step, z from it on
    double *part = g + (size_t)C * T;                                     // [Q][FGN_WAVES]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int row = gamma_row[blockIdx.x];
    row = row < 0 ? 0 : (row >= U ? U - 1 : row);                         // never read outside gamma, whatever gamma_row holds
    const double *gr = gamma + (int64_t)row * T;
    const double *zr = z + (int64_t)blockIdx.x * T * C;
    double *outr = out + (int64_t)blockIdx.x * T * C;
    double v = gr[0];
    const double s0 = sqrt(v);
    for (int i = tid; i < T; i += FGN_THREADS) {
        gam[i] = gr[i];
        phi[i] = 0.0;
    }
    for (int i = tid; i < T * C; i += FGN_THREADS) g[i] = i < C ? s0 * zr[i] : zr[i];
    __syncthreads();
    for (int n = 1; n < T; ++n) {
        double acc[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = 0.0;
        for (int j = 1 + tid; j < n; j += FGN_THREADS) {
            const double p = phi[j], pr = phi[n - j];
            acc[0] = acc[0] + p * gam[n - j];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double gv = g[(n - j) * C + c];
                acc[1 + c] = acc[1 + c] + p * gv;
                acc[1 + C + c] = acc[1 + C + c] + pr * gv;
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = wave_sum_f64(acc[q]);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < Q; ++q) part[q * FGN_WAVES + wave] = acc[q];
        }
        __syncthreads();                                                  // the wave sums are visible; phi and g were only read
#pragma unroll
        for (int q = 0; q < Q; ++q)
            acc[q] = (part[q * FGN_WAVES] + part[q * FGN_WAVES + 1]) + (part[q * FGN_WAVES + 2] + part[q * FGN_WAVES + 3]);
        const double kappa = (gam[n] - acc[0]) / v;
        v = v * (1.0 - kappa * kappa);
        const double sv = sqrt(v);                                        // in every thread: no divergent sqrt in wave 0
        if (tid < C) {                                                    // thread c finishes axis c
            double b = acc[1], r = acc[1 + C];
#pragma unroll
            for (int c = 1; c < C; ++c) {
                b = tid == c ? acc[1 + c] : b;
                r = tid == c ? acc[1 + C + c] : r;
            }
            const double m = (b - kappa * r) + kappa * g[tid];
            g[n * C + tid] = m + sv * g[n * C + tid];
        }
        for (int j = 1 + tid; 2 * j <= n; j += FGN_THREADS) {             // the pair (j, n - j) belongs to this thread alone
            const double a = phi[j], b = phi[n - j];
            phi[j] = a - kappa * b;
            phi[n - j] = b - kappa * a;
        }
        if (tid == FGN_THREADS - 1) phi[n] = kappa;
        __syncthreads();                                                  // phi, g[n] complete; part may be overwritten
    }
    for (int i = tid; i < T * C; i += FGN_THREADS) outr[i] = g[i];
}

template <int C>
int fgn_launch(const double *z, const double *gamma, const int *gamma_row, int N, int T, int U, double *out, hipStream_t s) {
    const size_t bytes = fgn_lds_doubles(T, C) * sizeof(double);
    auto kern = fgn_kernel<C>;
    if (bytes > 48 * 1024)
        MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(kern, dim3((unsigned)N), dim3(FGN_THREADS), bytes, s, z, gamma, gamma_row, U, T, out);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int mivit_fgn(const double *z, const double *gamma, const int *gamma_row, int N, int T, int C, int U, double *out,
                         void *stream) {
    MIVIT_CHECK(N >= 0 && T >= 0 && U >= 0, "fgn: N = %d, T = %d, U = %d: negative size", N, T, U);
    MIVIT_CHECK(C >= 1 && C <= FGN_MAX_C, "fgn: C = %d axes, 1 .. %d are supported", C, FGN_MAX_C);
    MIVIT_CHECK(T <= FGN_MAX_T, "fgn: T = %d steps, the limit is %d (the recursion's state lives in LDS)", T, FGN_MAX_T);
    if (N == 0 || T == 0) return 0;
    MIVIT_CHECK(U >= 1, "fgn: no autocovariance row (U = 0) for %d trajectories", N);
    MIVIT_CHECK(z && gamma && gamma_row && out, "fgn: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (C) {
        case 1: return fgn_launch<1>(z, gamma, gamma_row, N, T, U, out, s);
        case 2: return fgn_launch<2>(z, gamma, gamma_row, N, T, U, out, s);
        case 3: return fgn_launch<3>(z, gamma, gamma_row, N, T, U, out, s);
        default: return fgn_launch<4>(z, gamma, gamma_row, N, T, U, out, s);
    }
}
