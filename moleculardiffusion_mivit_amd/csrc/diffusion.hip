// From a linked movie to what the reference compares: the classical MSD estimate of the diffusion coefficient per track
// (helpers/helpersMSD.py:7-26 mean_square_displacement, :110-129 estimateDfromMSDs, :131-157 estimateDfromMSDsWeighted) and the
// normalised patch sequences a trained MiViT consumes (helpers/helpersTracking.py:513-550 extract_particle_patches followed by
// helpers/helpersGeneration.py:356-400 normalize_images).  Input is the detections table sorted by track (helpers/tracking.py::
// tracks_table_by_track).
//
// mivit_track_msd, one launch: one workgroup of 256 threads per track, one thread per lag, striding over the lags.  The
// positions of a track of up to MSD_LDS_ROWS rows are staged in LDS (16 bytes a row, 64 KiB); a longer track reads them
// through the cache with the same arithmetic.  Every sum runs in ascending index in one thread, so the result does not depend
// on the number of threads or on scheduling and equals the numpy restatement (helpers/msd.py::track_msd) bitwise.  The two
// estimates are reduced over the lags by thread 0 in ascending lag: O(L) after the O(L^2) of the lags.
//
// mivit_track_sequences, one launch: a pure gather, one thread per OUTPUT element in the output's own order ([n_seq, T, P, P]
// flat), so the 64 lanes of a wave store 256 consecutive bytes; the reads are runs of P consecutive pixels of a frame.
// Pixels outside the frame read as 0 before the normalisation, (v - lo) / denom with an IEEE fp32 division.
//
// No contraction into FMA: both kernels agree bitwise with their host statements.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int MSD_THREADS = 256;
constexpr int MSD_LDS_ROWS = 4096;    // 2 doubles a row: the 64 KiB of LDS a workgroup gets without asking (ops.MSD_LDS_ROWS)
constexpr int SEQ_THREADS = 256;
constexpr int SEQ_MAX_BLOCKS = 1 << 20;

// msd[tau] of one track: the positions p [L, 2] are in LDS or in global memory, the arithmetic is the same
__device__ __forceinline__ double msd_lag(const double *p, int L, int tau) {
    double s = 0.0;
    for (int i = 0; i < L - tau; ++i) {
        const double dy = p[2 * (i + tau)] - p[2 * i], dx = p[2 * (i + tau) + 1] - p[2 * i + 1];
        s = s + (dy * dy + dx * dx);
    }
    return s / (double)(L - tau);
}

__global__ __launch_bounds__(MSD_THREADS) void df_msd_kernel(const double *__restrict__ pos, int N,
                                                             const int *__restrict__ offsets, double dt, int max_lag, int Lmax,
                                                             double *__restrict__ msd, double *__restrict__ d_lstsq,
                                                             double *__restrict__ d_weighted) {
    __shared__ double p_lds[2 * MSD_LDS_ROWS];
    const int k = blockIdx.x, tid = threadIdx.x;
    int a = offsets[k], b = offsets[k + 1];
    a = a < 0 ? 0 : (a > N ? N : a);                                      // never read outside pos, whatever offsets holds
    b = b < a ? a : (b > N ? N : b);
    const int L = b - a;
    int M = L - 1;
    if (max_lag > 0 && M > max_lag) M = max_lag;
    if (M > Lmax - 1) M = Lmax - 1;                                       // never write outside the row
    const double *p = pos + (int64_t)a * 2;
    double *row = msd + (int64_t)k * Lmax;
    const bool staged = L <= MSD_LDS_ROWS;                                // uniform over the workgroup
    if (staged) {
        for (int i = tid; i < 2 * L; i += MSD_THREADS) p_lds[i] = p[i];
        __syncthreads();
    }
    for (int tau = tid; tau < Lmax; tau += MSD_THREADS) {
        double v = 0.0;
        if (tau >= 1 && tau <= M) v = staged ? msd_lag(p_lds, L, tau) : msd_lag(p, L, tau);
        row[tau] = v;
    }
    __syncthreads();                                                      // the row is complete and visible to thread 0
    if (tid != 0) return;
    double dl = NAN, dw = NAN;
    if (M >= 1) {
        double num = 0.0, den = 0.0, w = 0.0;
        for (int tau = 1; tau <= M; ++tau) {
            const double t = (double)tau * dt, m = row[tau];
            num = num + t * m;
            den = den + t * t;
            w = w + (m / (double)tau) * (double)(M + 1 - tau);
        }
        dl = num / den / 4.0;
        dw = w / ((double)(M + 1) * (double)(M + 2) / 2.0) / 4.0;
    }
    d_lstsq[k] = dl;
    d_weighted[k] = dw;
}

__global__ __launch_bounds__(SEQ_THREADS) void df_seq_kernel(const float *__restrict__ movie, int F, int H, int W,
                                                             const int *__restrict__ frame, const int *__restrict__ ys,
                                                             const int *__restrict__ xs, int N, const int *__restrict__ seq_row,
                                                             int T, int P, float lo, float denom, int normalize, int64_t total,
                                                             float *__restrict__ seq) {
    const int half = P / 2, PP = P * P;
    for (int64_t o = (int64_t)blockIdx.x * SEQ_THREADS + threadIdx.x; o < total; o += (int64_t)gridDim.x * SEQ_THREADS) {
        const int64_t patch = o / PP;
        const int pix = (int)(o - patch * PP), iy = pix / P, ix = pix - iy * P;
        const int64_t s = patch / T;
        const int t = (int)(patch - s * T);
        const int64_t r = (int64_t)seq_row[s] + t;
        float v = 0.f;
        bool live = false;
        if (r >= 0 && r < N) {
            const int f = frame[r];
            if (f >= 0 && f < F) {
                live = true;
                const int64_t py = (int64_t)ys[r] + (iy - half), px = (int64_t)xs[r] + (ix - half);
                if (py >= 0 && py < H && px >= 0 && px < W) v = movie[((int64_t)f * H + py) * W + px];
            }
        }
        if (live && normalize) v = (v - lo) / denom;
        seq[o] = v;
    }
}

}  // namespace

extern "C" int mivit_track_msd(const double *pos, int N, const int *offsets, int n_tracks, double dt, int max_lag, int Lmax,
                               double *msd, double *d_lstsq, double *d_weighted, void *stream) {
    MIVIT_CHECK(N >= 0, "track_msd: N = %d < 0", N);
    MIVIT_CHECK(n_tracks >= 0, "track_msd: n_tracks = %d < 0", n_tracks);
    MIVIT_CHECK(max_lag >= 0, "track_msd: max_lag = %d < 0 (0 means all lags)", max_lag);
    MIVIT_CHECK(Lmax >= 0, "track_msd: rows of %d lags", Lmax);
    MIVIT_CHECK(!(dt != dt), "track_msd: dt is NaN");
    if (n_tracks == 0) return 0;
    MIVIT_CHECK(offsets && d_lstsq && d_weighted, "track_msd: null pointer");
    MIVIT_CHECK((pos || N == 0) && (msd || Lmax == 0), "track_msd: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(df_msd_kernel, dim3((unsigned)n_tracks), dim3(MSD_THREADS), 0, static_cast<hipStream_t>(stream), pos, N,
                       offsets, dt, max_lag, Lmax, msd, d_lstsq, d_weighted);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_track_sequences(const float *movie, int F, int H, int W, const int *frame, const int *y, const int *x,
                                     int N, const int *seq_row, int n_seq, int T, int P, float lo, float denom, int normalize,
                                     float *seq, void *stream) {
    MIVIT_CHECK(F >= 0 && H >= 0 && W >= 0, "track_sequences: movie of %d x %d x %d", F, H, W);
    MIVIT_CHECK(N >= 0 && n_seq >= 0, "track_sequences: N = %d, n_seq = %d", N, n_seq);
    MIVIT_CHECK(T >= 1, "track_sequences: sequence length %d < 1", T);
    MIVIT_CHECK(P >= 3 && P <= 15 && P % 2 == 1, "track_sequences: patch side %d (odd, 3 .. 15)", P);
    MIVIT_CHECK(!normalize || (denom != 0.f && denom == denom && lo == lo), "track_sequences: lo = %g, denom = %g", (double)lo,
                (double)denom);
    if (n_seq == 0) return 0;
    MIVIT_CHECK(seq_row && seq, "track_sequences: null pointer");
    MIVIT_CHECK((frame && y && x) || N == 0, "track_sequences: null pointer");
    MIVIT_CHECK(movie || (int64_t)F * H * W == 0, "track_sequences: null pointer");
    const int64_t total = (int64_t)n_seq * T * P * P;
    int64_t blocks = (total + SEQ_THREADS - 1) / SEQ_THREADS;
    if (blocks > SEQ_MAX_BLOCKS) blocks = SEQ_MAX_BLOCKS;
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(df_seq_kernel, dim3((unsigned)blocks), dim3(SEQ_THREADS), 0, static_cast<hipStream_t>(stream), movie, F, H,
                       W, frame, y, x, N, seq_row, T, P, lo, denom, normalize, total, seq);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
