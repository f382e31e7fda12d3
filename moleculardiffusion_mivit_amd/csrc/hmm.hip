// Diffusion states shared across tracks: the E-step (scaled forward-backward) and the Viterbi path of a hidden Markov model
// over the squared increments of every track of a movie (no counterpart in the reference; the model is the inverse of
// andi_datasets' multi_state, the estimator that of vbSPT, Persson et al., Nat. Methods 10, 265 (2013), in its maximum-
// likelihood form).  include/mivit_hip.h spells the arithmetic out; helpers/msd.py restates it in numpy.
//
// Both kernels: a GROUP OF 8 LANES owns one track, lane j of the group is state j, a workgroup of 64 threads (one wave) holds
// 8 tracks.  The recurrence is sequential along a track and independent between tracks; what crosses lanes (alpha_{t-1}[i]
// forward, w_{t+1}[j] and alpha_t[i] backward, delta_{t-1}[i] and the back-pointer of the state on the path in Viterbi) goes
// through width-8 shuffles, K of them per lane and step, summed in ascending index.  Lane j keeps column j of xi, g_sum[j],
// gq_sum[j] in registers (loops over 8 fully unrolled and guarded by i < K, K a template parameter: no register array is
// indexed dynamically, and no guard is a run-time branch that lanes of different tracks would have to agree on).  No
// LDS, no atomics, no s_barrier.  alpha_t[j] is stored in gamma[row][j] on the way forward and overwritten by gamma_t[j] on
// the way back, b_j(q_t) / c_t in the workspace, the back-pointers in theirs: a lane reads back from global memory ONLY WHAT
// IT WROTE ITSELF, so no fence is needed, and a track has no maximum length.  Groups whose tracks have ended sit masked out
// while the others of the wave continue; every group shuffles only within itself, and the mapping of a track to its lanes
// does not change what they compute: a track's outputs are bitwise the same alone, anywhere in a batch and in every launch.
//
// No contraction into FMA, as in segment.hip.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int HMM_THREADS = 64;       // one wave
constexpr int HMM_GROUP = 8;          // lanes of a track = the most states (ops.MARKOV_MAX_K)
constexpr int HMM_MAX_K = 8;
constexpr double HMM_LOG_2PI = 1.8378770664093453;                        // np.log(2 * np.pi)

__device__ __forceinline__ double grp(double x, int i) { return __shfl(x, i, HMM_GROUP); }
__device__ __forceinline__ int grp(int x, int i) { return __shfl(x, i, HMM_GROUP); }

// q_t of the increment from row t to row t + 1
__device__ __forceinline__ double hmm_q(const double *__restrict__ p, int t) {
    const double dy = p[2 * (t + 1)] - p[2 * t], dx = p[2 * (t + 1) + 1] - p[2 * t + 1];
    return dy * dy + dx * dx;
}

template <int K>
__global__ __launch_bounds__(HMM_THREADS) void hmm_estep_kernel(const double *__restrict__ pos, int N,
                                                                const int *__restrict__ offsets, int n_tracks,
                                                                const double *__restrict__ v, const double *__restrict__ A,
                                                                const double *__restrict__ pi, double *gamma,
                                                                int *__restrict__ state, double *__restrict__ xi_out,
                                                                double *__restrict__ g_sum, double *__restrict__ gq_sum,
                                                                double *__restrict__ g_first, double *__restrict__ loglik,
                                                                double *ws) {
    const int k = blockIdx.x * (HMM_THREADS / HMM_GROUP) + (threadIdx.x >> 3), j = threadIdx.x & 7;
    if (k >= n_tracks) return;                                            // uniform over the group
    const bool on = j < K;                                                // lanes K .. 7 run along on zeros and store nothing
    int a = offsets[k], b = offsets[k + 1];
    a = a < 0 ? 0 : (a > N ? N : a);                                      // never read or write outside [0, N), whatever offsets holds
    b = b < a ? a : (b > N ? N : b);
    const int T = b - a - 1;
    double *xk = xi_out + (int64_t)k * K * K;
    if (T < 1) {                                                          // uniform over the group
        if (on) {
            if (T == 0) gamma[(int64_t)a * K + j] = NAN;
#pragma unroll
            for (int i = 0; i < HMM_MAX_K; ++i)
                if (i < K) xk[i * K + j] = NAN;
            g_sum[(int64_t)k * K + j] = NAN;
            gq_sum[(int64_t)k * K + j] = NAN;
            g_first[(int64_t)k * K + j] = NAN;
        }
        if (j == 0) {
            if (T == 0) state[a] = -1;
            loglik[k] = NAN;
        }
        return;
    }
    double vmax = v[0];
    for (int i = 1; i < K; ++i) vmax = v[i] > vmax ? v[i] : vmax;
    const double tvmax = 2.0 * vmax;
    const double vj = on ? v[j] : vmax, tvj = 2.0 * vj, pij = on ? pi[j] : 0.0;
    double Ac0 = 0.0, Ac1 = 0.0, Ac2 = 0.0, Ac3 = 0.0, Ac4 = 0.0, Ac5 = 0.0, Ac6 = 0.0, Ac7 = 0.0;       // A[i][j]: column j
    double Ar0 = 0.0, Ar1 = 0.0, Ar2 = 0.0, Ar3 = 0.0, Ar4 = 0.0, Ar5 = 0.0, Ar6 = 0.0, Ar7 = 0.0;       // A[j][i]: row j
#define HMM_LOAD_A(i)                \
    if (on && i < K) {               \
        Ac##i = A[i * K + j];        \
        Ar##i = A[j * K + i];        \
    }
    HMM_LOAD_A(0) HMM_LOAD_A(1) HMM_LOAD_A(2) HMM_LOAD_A(3) HMM_LOAD_A(4) HMM_LOAD_A(5) HMM_LOAD_A(6) HMM_LOAD_A(7)
#undef HMM_LOAD_A
    const double *p = pos + (int64_t)a * 2;
    double *gk = gamma + (int64_t)a * K + j;                              // gk[t * K]: this lane's entry of row a + t
    double *wk = ws + (int64_t)a * K + j;

    // forward: alpha_t into gamma, b / c_t into the workspace
    double alpha = 0.0, slc = 0.0, sm = 0.0, cbad = 1.0;
    bool dead = false;
    for (int t = 0; t < T; ++t) {
        const double q = hmm_q(p, t);
        const double m = q / tvmax;
        const double bj = exp(-(q / tvj - m)) / vj;
        double x;
        if (t == 0) {
            x = pij * bj;
        } else {
            double s = 0.0;
#define HMM_PRED(i) \
    if (i < K) s = s + grp(alpha, i) * Ac##i;
            HMM_PRED(0) HMM_PRED(1) HMM_PRED(2) HMM_PRED(3) HMM_PRED(4) HMM_PRED(5) HMM_PRED(6) HMM_PRED(7)
#undef HMM_PRED
            x = s * bj;
        }
        double c = 0.0;
#define HMM_NORM(i) \
    if (i < K) c = c + grp(x, i);
        HMM_NORM(0) HMM_NORM(1) HMM_NORM(2) HMM_NORM(3) HMM_NORM(4) HMM_NORM(5) HMM_NORM(6) HMM_NORM(7)
#undef HMM_NORM
        if (!(c > 0.0 && c < INFINITY)) {                                 // the same c in every lane: uniform over the group
            dead = true;
            cbad = c;
            break;
        }
        alpha = x / c;
        slc = slc + log(c);
        sm = sm + m;
        if (on) {
            gk[(int64_t)t * K] = alpha;
            wk[(int64_t)t * K] = bj / c;
        }
    }
    if (dead) {                                                           // underflow to 0 (-inf) or a NaN / inf position (NaN)
        if (on) {
            for (int t = 0; t <= T; ++t) gk[(int64_t)t * K] = NAN;
#pragma unroll
            for (int i = 0; i < HMM_MAX_K; ++i)
                if (i < K) xk[i * K + j] = NAN;
            g_sum[(int64_t)k * K + j] = NAN;
            gq_sum[(int64_t)k * K + j] = NAN;
            g_first[(int64_t)k * K + j] = NAN;
        }
        for (int t = j; t <= T; t += HMM_GROUP) state[a + t] = -1;
        if (j == 0) loglik[k] = cbad == 0.0 ? -INFINITY : NAN;
        return;
    }

    // backward: beta in registers, gamma over alpha, the statistics in registers
    double beta = 1.0, gs = 0.0, gqs = 0.0, gam = 0.0;
    double xi0 = 0.0, xi1 = 0.0, xi2 = 0.0, xi3 = 0.0, xi4 = 0.0, xi5 = 0.0, xi6 = 0.0, xi7 = 0.0;       // xi[i][j], lane j
    int best = 0;
    for (int t = T - 1; t >= 0; --t) {
        alpha = on ? gk[(int64_t)t * K] : 0.0;
        if (t < T - 1) {
            const double w = (on ? wk[(int64_t)(t + 1) * K] : 0.0) * beta;                                // w_{t+1}[j]
            double nb = 0.0;
#define HMM_BACK(i)                                 \
    if (i < K) {                                    \
        nb = nb + Ar##i * grp(w, i);                \
        xi##i = xi##i + (grp(alpha, i) * Ac##i) * w; \
    }
            HMM_BACK(0) HMM_BACK(1) HMM_BACK(2) HMM_BACK(3) HMM_BACK(4) HMM_BACK(5) HMM_BACK(6) HMM_BACK(7)
#undef HMM_BACK
            beta = nb;
        }
        gam = alpha * beta;
        const double q = hmm_q(p, t);
        gs = gs + gam;
        gqs = gqs + gam * q;
        double bg = grp(gam, 0);
        best = 0;
#define HMM_ARGMAX(i)                  \
    if (i < K) {                       \
        const double og = grp(gam, i); \
        if (og > bg) {                 \
            bg = og;                   \
            best = i;                  \
        }                              \
    }
        HMM_ARGMAX(1) HMM_ARGMAX(2) HMM_ARGMAX(3) HMM_ARGMAX(4) HMM_ARGMAX(5) HMM_ARGMAX(6) HMM_ARGMAX(7)
#undef HMM_ARGMAX
        if (on) gk[(int64_t)t * K] = gam;
        if (j == 0) state[a + t] = best;
        if (t == T - 1) {                                                 // the last row repeats the row before it
            if (on) gk[(int64_t)T * K] = gam;
            if (j == 0) state[a + T] = best;
        }
    }
    if (on) {
#define HMM_XI(i) \
    if (i < K) xk[i * K + j] = xi##i;
        HMM_XI(0) HMM_XI(1) HMM_XI(2) HMM_XI(3) HMM_XI(4) HMM_XI(5) HMM_XI(6) HMM_XI(7)
#undef HMM_XI
        g_sum[(int64_t)k * K + j] = gs;
        gq_sum[(int64_t)k * K + j] = gqs;
        g_first[(int64_t)k * K + j] = gam;                                // gamma_0: the last of the descending loop
    }
    if (j == 0) loglik[k] = (slc - sm) - (double)T * HMM_LOG_2PI;
}

template <int K>
__global__ __launch_bounds__(HMM_THREADS) void hmm_viterbi_kernel(const double *__restrict__ pos, int N,
                                                                  const int *__restrict__ offsets, int n_tracks,
                                                                  const double *__restrict__ v, const double *__restrict__ logv,
                                                                  const double *__restrict__ logA,
                                                                  const double *__restrict__ logpi, int *__restrict__ state,
                                                                  double *__restrict__ logp, unsigned char *bp) {
    const int k = blockIdx.x * (HMM_THREADS / HMM_GROUP) + (threadIdx.x >> 3), j = threadIdx.x & 7;
    if (k >= n_tracks) return;
    const bool on = j < K;
    int a = offsets[k], b = offsets[k + 1];
    a = a < 0 ? 0 : (a > N ? N : a);
    b = b < a ? a : (b > N ? N : b);
    const int T = b - a - 1;
    if (T < 1) {
        if (j == 0) {
            if (T == 0) state[a] = -1;
            logp[k] = NAN;
        }
        return;
    }
    const double tvj = on ? 2.0 * v[j] : 2.0, lvj = on ? logv[j] : 0.0, lpj = on ? logpi[j] : 0.0;
    double La0 = 0.0, La1 = 0.0, La2 = 0.0, La3 = 0.0, La4 = 0.0, La5 = 0.0, La6 = 0.0, La7 = 0.0;       // logA[i][j]: column j
#define HMM_LOAD_LA(i) \
    if (on && i < K) La##i = logA[i * K + j];
    HMM_LOAD_LA(0) HMM_LOAD_LA(1) HMM_LOAD_LA(2) HMM_LOAD_LA(3) HMM_LOAD_LA(4) HMM_LOAD_LA(5) HMM_LOAD_LA(6) HMM_LOAD_LA(7)
#undef HMM_LOAD_LA
    const double *p = pos + (int64_t)a * 2;
    unsigned char *bk = bp + (int64_t)a * HMM_GROUP + j;                  // bk[t * 8]: this lane's back-pointer of increment t
    double delta = 0.0;
    for (int t = 0; t < T; ++t) {
        const double q = hmm_q(p, t);
        const double lb = -(q / tvj) - lvj;
        if (t == 0) {
            delta = lpj + lb;
        } else {
            double bv = grp(delta, 0) + La0;
            int bi = 0;
#define HMM_STEP(i)                                   \
    if (i < K) {                                      \
        const double cand = grp(delta, i) + La##i;    \
        if (cand > bv) {                              \
            bv = cand;                                \
            bi = i;                                   \
        }                                             \
    }
            HMM_STEP(1) HMM_STEP(2) HMM_STEP(3) HMM_STEP(4) HMM_STEP(5) HMM_STEP(6) HMM_STEP(7)
#undef HMM_STEP
            delta = bv + lb;
            bk[(int64_t)t * HMM_GROUP] = (unsigned char)bi;               // every lane its own byte, lanes K .. 7 included
        }
    }
    double bv = grp(delta, 0);
    int s = 0;
#define HMM_END(i)                         \
    if (i < K) {                           \
        const double cand = grp(delta, i); \
        if (cand > bv) {                   \
            bv = cand;                     \
            s = i;                         \
        }                                  \
    }
    HMM_END(1) HMM_END(2) HMM_END(3) HMM_END(4) HMM_END(5) HMM_END(6) HMM_END(7)
#undef HMM_END
    if (j == 0) {
        logp[k] = bv;
        state[a + T] = s;                                                 // the last row repeats the row before it
        state[a + T - 1] = s;
    }
    for (int t = T - 1; t > 0; --t) {                                     // s is the same in every lane of the group
        const int mine = bk[(int64_t)t * HMM_GROUP];                      // written by this lane
        s = grp(mine, s) & 7;
        if (j == 0) state[a + t - 1] = s;
    }
}

// K is a template parameter: the guards i < K of the unrolled loops are decided at compile time
#define HMM_DISPATCH(kernel, ...)                                                                                          \
    switch (K) {                                                                                                           \
        case 1: hipLaunchKernelGGL(kernel<1>, grid, dim3(HMM_THREADS), 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(HMM_THREADS), 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL(kernel<3>, grid, dim3(HMM_THREADS), 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break; \
        case 4: hipLaunchKernelGGL(kernel<4>, grid, dim3(HMM_THREADS), 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break; \
        case 5: hipLaunchKernelGGL(kernel<5>, grid, dim3(HMM_THREADS), 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break; \
        case 6: hipLaunchKernelGGL(kernel<6>, grid, dim3(HMM_THREADS), 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break; \
        case 7: hipLaunchKernelGGL(kernel<7>, grid, dim3(HMM_THREADS), 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break; \
        default: hipLaunchKernelGGL(kernel<8>, grid, dim3(HMM_THREADS), 0, static_cast<hipStream_t>(stream), __VA_ARGS__); break; \
    }

}  // namespace

extern "C" int mivit_hmm_estep(const double *pos, int N, const int *offsets, int n_tracks, int K, const double *v, const double *A,
                               const double *pi, double *gamma, int *state, double *xi, double *g_sum, double *gq_sum,
                               double *g_first, double *loglik, double *workspace, void *stream) {
    MIVIT_CHECK(N >= 0 && n_tracks >= 0, "hmm_estep: N = %d, n_tracks = %d: negative size", N, n_tracks);
    MIVIT_CHECK(K >= 1 && K <= HMM_MAX_K, "hmm_estep: K = %d states, 1 .. %d are supported", K, HMM_MAX_K);
    if (n_tracks == 0) return 0;
    MIVIT_CHECK(offsets && v && A && pi && xi && g_sum && gq_sum && g_first && loglik, "hmm_estep: null pointer");
    MIVIT_CHECK((pos && gamma && state && workspace) || N == 0, "hmm_estep: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    const dim3 grid((unsigned)ceil_div(n_tracks, HMM_THREADS / HMM_GROUP));
    HMM_DISPATCH(hmm_estep_kernel, pos, N, offsets, n_tracks, v, A, pi, gamma, state, xi, g_sum, gq_sum, g_first, loglik, workspace)
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_hmm_viterbi(const double *pos, int N, const int *offsets, int n_tracks, int K, const double *v,
                                 const double *logv, const double *logA, const double *logpi, int *state, double *logp,
                                 unsigned char *workspace, void *stream) {
    MIVIT_CHECK(N >= 0 && n_tracks >= 0, "hmm_viterbi: N = %d, n_tracks = %d: negative size", N, n_tracks);
    MIVIT_CHECK(K >= 1 && K <= HMM_MAX_K, "hmm_viterbi: K = %d states, 1 .. %d are supported", K, HMM_MAX_K);
    if (n_tracks == 0) return 0;
    MIVIT_CHECK(offsets && v && logv && logA && logpi && logp, "hmm_viterbi: null pointer");
    MIVIT_CHECK((pos && state && workspace) || N == 0, "hmm_viterbi: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    const dim3 grid((unsigned)ceil_div(n_tracks, HMM_THREADS / HMM_GROUP));
    HMM_DISPATCH(hmm_viterbi_kernel, pos, N, offsets, n_tracks, v, logv, logA, logpi, state, logp, workspace)
    MIVIT_LAUNCH_CHECK();
    return 0;
}
