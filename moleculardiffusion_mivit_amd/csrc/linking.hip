// Frame-to-frame linking of a whole movie on the GPU: the counterpart of the reference's link_particles
// (helpers/helpersTracking.py:123-177, one scipy.optimize.linear_sum_assignment per frame) and of the id book-keeping of its
// track_particles (:225-336).  Input is what mivit_dog_peaks leaves on the device.
//
// mivit_link_frames, one launch: one workgroup of ONE wave per frame f, which solves the full rectangular assignment between
// the n0 detections of frame f - 1 and the n1 of frame f on the Euclidean distance and only then drops the links longer than
// max_distance (solve first, filter afterwards, as the reference does).
//   Solver: shortest augmenting paths with dual variables (Jonker-Volgenant as stated by Crouse, the algorithm scipy uses), fp64.
//   Roles: the side with FEWER detections plays "rows" (one augmentation per row); with n0 == n1 the rows are frame f - 1.
//   Rows are augmented in ascending index.  The cost sqrt(dy^2 + dx^2) is recomputed from the coordinates in LDS whenever it
//   is needed (a 512 x 512 fp64 matrix would be 2 MiB); the state is a handful of arrays of n entries in LDS: coordinates of
//   both sides, the duals u / v, the shortest path cost and predecessor per column, the two matchings, the two visited sets.
//   Columns are spread over the 64 lanes; "closest unvisited column" is a butterfly minimum over the wave on the key
//   (path cost, column already matched?, column index): among equal path costs a free column wins (the search ends there),
//   then the lower index.  The key is a total order, so the result does not depend on lane order or scheduling.
//   One wave, because the search is a chain of dependent steps that each end in that minimum: within a wave it needs no
//   barrier that waits for anybody, and the F - 1 problems of a movie fill the machine side by side.
//
// mivit_chain_tracks, one workgroup: the sequential hand-down of track ids.  Per frame, a linked detection inherits its
// partner's id (kept in LDS from the frame before), an unlinked one takes next_id + its rank among the unlinked ones of the
// frame in ascending detection index (a ballot scan per 256 detections); frame 0 and every movie_start frame open one track
// per detection.  The length of each track is carried along and stored under its id.
//
// No contraction into FMA: path costs and duals agree bitwise with the host restatement (helpers/tracking.py).
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int LK_MAX_N = 1024;        // detections per frame: 54 bytes of LDS each, 54 KiB
constexpr int LK_WAVE = 64;
constexpr int LK_MATCHED = 1 << 30;   // key bit: the column already has a row
constexpr int CH_THREADS = 256;

__host__ __device__ constexpr size_t lk_lds_bytes(int cap) {
    // 3 double arrays, 7 int arrays, 2 byte arrays (cap rounded up to 8 keeps every array aligned)
    return (size_t)((cap + 7) / 8 * 8) * (3 * sizeof(double) + 7 * sizeof(int) + 2);
}

struct LkKey {
    double cost;
    int code;                          // LK_MATCHED | column
};

__device__ __forceinline__ bool lk_less(double c, int code, const LkKey &b) {
    return c < b.cost || (c == b.cost && code < b.code);
}

__global__ __launch_bounds__(LK_WAVE) void lk_link_kernel(const int *__restrict__ coords, const int *__restrict__ count,
                                                          const unsigned char *__restrict__ movie_start, int cap,
                                                          double max_distance, int *__restrict__ link) {
    extern __shared__ double lk_lds[];
    const int C = (cap + 7) / 8 * 8;
    double *u = lk_lds, *v = u + C, *spc = v + C;
    int *ry = reinterpret_cast<int *>(spc + C), *rx = ry + C, *cy = rx + C, *cx = cy + C;
    int *path = cx + C, *col4row = path + C, *row4col = col4row + C;
    unsigned char *SR = reinterpret_cast<unsigned char *>(row4col + C), *SC = SR + C;
    const int f = blockIdx.x, lane = threadIdx.x;
    int *out = link + (int64_t)f * cap;
    int n0 = 0, n1 = 0;
    if (f > 0 && !(movie_start && movie_start[f])) {
        n0 = count[f - 1];
        n1 = count[f];
        n0 = n0 < 0 ? 0 : (n0 > cap ? cap : n0);
        n1 = n1 < 0 ? 0 : (n1 > cap ? cap : n1);
    }
    if (n0 == 0 || n1 == 0) {                                             // first frame of a movie, or nothing to link
        for (int j = lane; j < cap; j += LK_WAVE) out[j] = -1;
        return;
    }
    const bool rows_prev = n0 <= n1;                                      // the smaller side plays rows
    const int nr = rows_prev ? n0 : n1, nc = rows_prev ? n1 : n0;
    const int *rsrc = coords + (int64_t)(rows_prev ? f - 1 : f) * cap * 2;
    const int *csrc = coords + (int64_t)(rows_prev ? f : f - 1) * cap * 2;
    for (int i = lane; i < nr; i += LK_WAVE) {
        ry[i] = rsrc[2 * i];
        rx[i] = rsrc[2 * i + 1];
        u[i] = 0.0;
        col4row[i] = -1;
    }
    for (int j = lane; j < nc; j += LK_WAVE) {
        cy[j] = csrc[2 * j];
        cx[j] = csrc[2 * j + 1];
        v[j] = 0.0;
        row4col[j] = -1;
    }
    __syncthreads();
    for (int cur = 0; cur < nr; ++cur) {
        for (int i = lane; i < nr; i += LK_WAVE) SR[i] = 0;
        for (int j = lane; j < nc; j += LK_WAVE) {
            SC[j] = 0;
            spc[j] = INFINITY;
        }
        __syncthreads();
        double min_val = 0.0;
        int i = cur, sink = -1;
        // every pass visits one more column and at most cur of the nc >= nr columns are matched: a free one is reached
        // within cur + 1 passes.  The bound on the loop only keeps a corrupted input from spinning.
        for (int pass = 0; pass <= nc && sink < 0; ++pass) {
            if (lane == 0) SR[i] = 1;
            const double ui = u[i];
            const int iy = ry[i], ix = rx[i];
            LkKey best{INFINITY, INT32_MAX};
            for (int j = lane; j < nc; j += LK_WAVE) {
                if (SC[j]) continue;
                const double dy = (double)(iy - cy[j]), dx = (double)(ix - cx[j]);
                const double c = sqrt(dy * dy + dx * dx);
                const double r = ((min_val + c) - ui) - v[j];
                double s = spc[j];
                if (r < s) {
                    s = r;
                    spc[j] = r;
                    path[j] = i;
                }
                const int code = (row4col[j] >= 0 ? LK_MATCHED : 0) | j;
                if (lk_less(s, code, best)) best = LkKey{s, code};
            }
            for (int m = LK_WAVE / 2; m > 0; m >>= 1) {
                const double oc = __shfl_xor(best.cost, m, LK_WAVE);
                const int ok = __shfl_xor(best.code, m, LK_WAVE);
                if (lk_less(oc, ok, best)) best = LkKey{oc, ok};
            }
            if (best.code == INT32_MAX) break;                            // no column left: cannot happen with nr <= nc
            min_val = best.cost;
            const int j = best.code & (LK_MATCHED - 1);
            if (best.code & LK_MATCHED) i = row4col[j];
            else sink = j;
            if (lane == 0) SC[j] = 1;
            __syncthreads();
        }
        if (sink < 0) break;                                              // uniform: every lane holds the same sink
        // dual update (Crouse, step 4), each entry by one lane
        for (int r = lane; r < nr; r += LK_WAVE)
            if (SR[r]) u[r] = r == cur ? u[r] + min_val : u[r] + (min_val - spc[col4row[r]]);
        for (int j = lane; j < nc; j += LK_WAVE)
            if (SC[j]) v[j] = v[j] - (min_val - spc[j]);
        __syncthreads();
        if (lane == 0) {                                                  // augment along the predecessors
            int j = sink;
            for (int step = 0; step <= nr; ++step) {
                const int r = path[j];
                row4col[j] = r;
                const int t = col4row[r];
                col4row[r] = j;
                j = t;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    // filter afterwards: a link longer than max_distance is dropped, its two ends stay unlinked.  Every entry of the frame's
    // row of `link` is written exactly once.
    for (int k = lane; k < cap; k += LK_WAVE) {
        int partner = -1;
        if (k < n1) {
            const int r = rows_prev ? row4col[k] : k, j = rows_prev ? k : col4row[k];
            if (r >= 0 && j >= 0) {
                const double dy = (double)(ry[r] - cy[j]), dx = (double)(rx[r] - cx[j]);
                if (sqrt(dy * dy + dx * dx) <= max_distance) partner = rows_prev ? r : j;
            }
        }
        out[k] = partner;
    }
}

__global__ __launch_bounds__(CH_THREADS) void lk_chain_kernel(const int *__restrict__ link, const int *__restrict__ count,
                                                               const unsigned char *__restrict__ movie_start, int F, int cap,
                                                               int *__restrict__ ids, int *__restrict__ lengths,
                                                               int *__restrict__ n_tracks) {
    extern __shared__ int ch_lds[];                                       // id and length so far, two frames each
    __shared__ int wave_total[2][CH_THREADS / LK_WAVE];
    int *id_buf = ch_lds, *len_buf = ch_lds + 2 * cap;
    const int tid = threadIdx.x, lane = tid & (LK_WAVE - 1), wave = tid / LK_WAVE;
    int next_id = 0, n_prev = 0, parity = 0;
    int n_next = count[0], l_next = tid < cap ? link[tid] : -1;           // the first chunk of a frame is fetched one frame ahead
    for (int f = 0; f < F; ++f) {
        int n = n_next;
        n = n < 0 ? 0 : (n > cap ? cap : n);
        const int l_first = l_next;
        if (f + 1 < F) {
            n_next = count[f + 1];
            l_next = tid < cap ? link[(int64_t)(f + 1) * cap + tid] : -1;
        }
        const bool fresh = f == 0 || (movie_start && movie_start[f]);
        int *id_cur = id_buf + (f & 1) * cap, *len_cur = len_buf + (f & 1) * cap;
        const int *id_prev = id_buf + ((f & 1) ^ 1) * cap, *len_prev = len_buf + ((f & 1) ^ 1) * cap;
        for (int base = 0; base < n; base += CH_THREADS) {
            const int j = base + tid;
            const bool valid = j < n;
            int l = -1;
            if (valid && !fresh) l = base == 0 ? l_first : link[(int64_t)f * cap + j];
            if (l >= n_prev) l = -1;                                      // never read past the previous frame
            const bool is_new = valid && l < 0;
            const unsigned long long mask = __ballot(is_new);
            const int before = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) wave_total[parity][wave] = __popcll(mask);
            __syncthreads();
            int off = before, total = 0;
            for (int w = 0; w < CH_THREADS / LK_WAVE; ++w) {
                const int t = wave_total[parity][w];
                if (w < wave) off += t;
                total += t;
            }
            parity ^= 1;
            if (valid) {
                const int id = is_new ? next_id + off : id_prev[l];
                const int len = is_new ? 1 : len_prev[l] + 1;
                id_cur[j] = id;
                len_cur[j] = len;
                ids[(int64_t)f * cap + j] = id;
                lengths[id] = len;                                        // later frames store the larger value after a barrier
            }
            next_id += total;
        }
        n_prev = n;
        __syncthreads();
    }
    if (tid == 0) n_tracks[0] = next_id;
}

}  // namespace

extern "C" int mivit_link_frames(const int *coords, const int *count, const unsigned char *movie_start, int F, int cap,
                                 double max_distance, int *link, void *stream) {
    MIVIT_CHECK(F >= 0, "link_frames: F = %d < 0", F);
    MIVIT_CHECK(cap >= 1 && cap <= LK_MAX_N, "link_frames: capacity of %d detections per frame (1 .. %d)", cap, LK_MAX_N);
    MIVIT_CHECK(!(max_distance != max_distance), "link_frames: max_distance is NaN");
    if (F == 0) return 0;
    MIVIT_CHECK(coords && count && link, "link_frames: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(lk_link_kernel, dim3((unsigned)F), dim3(LK_WAVE), lk_lds_bytes(cap), static_cast<hipStream_t>(stream),
                       coords, count, movie_start, cap, max_distance, link);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

extern "C" int mivit_chain_tracks(const int *link, const int *count, const unsigned char *movie_start, int F, int cap,
                                  int *ids, int *lengths, int *n_tracks, void *stream) {
    MIVIT_CHECK(F >= 0, "chain_tracks: F = %d < 0", F);
    MIVIT_CHECK(cap >= 1 && cap <= LK_MAX_N, "chain_tracks: capacity of %d detections per frame (1 .. %d)", cap, LK_MAX_N);
    MIVIT_CHECK(n_tracks, "chain_tracks: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (F == 0) {
        MIVIT_HIP(hipMemsetAsync(n_tracks, 0, sizeof(int), s));
        return 0;
    }
    MIVIT_CHECK(link && count && ids && lengths, "chain_tracks: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(lk_chain_kernel, dim3(1), dim3(CH_THREADS), (size_t)4 * cap * sizeof(int), s, link, count, movie_start,
                       F, cap, ids, lengths, n_tracks);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
