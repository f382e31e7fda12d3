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
// mivit_close_gaps, one small launch that clears the outputs and builds the open-end state from `link`, then one launch per
// pass g = 2 .. max_gap + 1 (shortest gaps first) of F one-wave workgroups: workgroup f compacts the open ends of frame f - g
// and the open starts of frame f into the solver's LDS arrays (two index maps lead back to detection indices), runs the same
// solver (lk_solve, shared with lk_link_kernel), filters by max_distance and records the accepted pairs.  Within a pass the
// workgroups are independent: workgroup f reads and writes the end state (has_succ) of frame f - g only and the start state
// (gap_frames) of frame f only, two separate arrays, so its writes never meet the reads of workgroup f + g.  Across passes
// the dependence is real, hence the separate launches on one stream.
//
// mivit_chain_tracks_gaps: lk_chain_kernel with a ring of max_gap + 2 frames of ids in LDS, so that a gap link of g frames
// finds its partner's id; lengths are counted with one integer atomic per detection (the array is cleared first).
//
// No contraction into FMA: path costs and duals agree bitwise with the host restatement (helpers/tracking.py).
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int LK_MAX_N = 1024;        // detections per frame: 54 bytes of LDS each, 54 KiB
constexpr int LK_WAVE = 64;
constexpr int LK_MATCHED = 1 << 30;   // key bit: the column already has a row
constexpr int CH_THREADS = 256;
constexpr int LK_MAX_GAP = 8;         // missed frames a gap link may bridge: the chain kernel's ring holds LK_MAX_GAP + 2 frames

__host__ __device__ constexpr size_t lk_lds_bytes(int cap) {
    // 3 double arrays, 7 int arrays, 2 byte arrays (cap rounded up to 8 keeps every array aligned)
    return (size_t)((cap + 7) / 8 * 8) * (3 * sizeof(double) + 7 * sizeof(int) + 2);
}

__host__ __device__ constexpr size_t gc_lds_bytes(int cap) {
    // the solver's arrays and two index maps: 63 488 bytes at cap = 1024, under the 64 KiB a launch gets without an attribute
    return lk_lds_bytes(cap) + (size_t)((cap + 7) / 8 * 8) * 2 * sizeof(int);
}

struct LkKey {
    double cost;
    int code;                          // LK_MATCHED | column
};

__device__ __forceinline__ bool lk_less(double c, int code, const LkKey &b) {
    return c < b.cost || (c == b.cost && code < b.code);
}

// The solver's state in LDS, carved from one dynamic allocation of lk_lds_bytes(cap) bytes.
struct LkLds {
    double *u, *v, *spc;
    int *ry, *rx, *cy, *cx, *path, *col4row, *row4col;
    unsigned char *SR, *SC;
};

__device__ __forceinline__ LkLds lk_carve(double *lds, int C) {
    LkLds L;
    L.u = lds, L.v = L.u + C, L.spc = L.v + C;
    L.ry = reinterpret_cast<int *>(L.spc + C), L.rx = L.ry + C, L.cy = L.rx + C, L.cx = L.cy + C;
    L.path = L.cx + C, L.col4row = L.path + C, L.row4col = L.col4row + C;
    L.SR = reinterpret_cast<unsigned char *>(L.row4col + C), L.SC = L.SR + C;
    return L;
}

// Exact assignment of the nr <= nc rows (ry, rx) to the columns (cy, cx) by one wave; u, v zeroed and col4row, row4col set
// to -1 by the caller, followed by a barrier.  Leaves the matching in col4row / row4col.
__device__ __forceinline__ void lk_solve(const LkLds &L, int nr, int nc, int lane) {
    double *u = L.u, *v = L.v, *spc = L.spc;
    const int *ry = L.ry, *rx = L.rx, *cy = L.cy, *cx = L.cx;
    int *path = L.path, *col4row = L.col4row, *row4col = L.row4col;
    unsigned char *SR = L.SR, *SC = L.SC;
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
}

__device__ __forceinline__ int lk_clamp_count(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

__global__ __launch_bounds__(LK_WAVE) void lk_link_kernel(const int *__restrict__ coords, const int *__restrict__ count,
                                                          const unsigned char *__restrict__ movie_start, int cap,
                                                          double max_distance, int *__restrict__ link) {
    extern __shared__ double lk_lds[];
    const LkLds L = lk_carve(lk_lds, (cap + 7) / 8 * 8);
    const int f = blockIdx.x, lane = threadIdx.x;
    int *out = link + (int64_t)f * cap;
    int n0 = 0, n1 = 0;
    if (f > 0 && !(movie_start && movie_start[f])) {
        n0 = lk_clamp_count(count[f - 1], cap);
        n1 = lk_clamp_count(count[f], cap);
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
        L.ry[i] = rsrc[2 * i];
        L.rx[i] = rsrc[2 * i + 1];
        L.u[i] = 0.0;
        L.col4row[i] = -1;
    }
    for (int j = lane; j < nc; j += LK_WAVE) {
        L.cy[j] = csrc[2 * j];
        L.cx[j] = csrc[2 * j + 1];
        L.v[j] = 0.0;
        L.row4col[j] = -1;
    }
    __syncthreads();
    lk_solve(L, nr, nc, lane);
    // filter afterwards: a link longer than max_distance is dropped, its two ends stay unlinked.  Every entry of the frame's
    // row of `link` is written exactly once.
    for (int k = lane; k < cap; k += LK_WAVE) {
        int partner = -1;
        if (k < n1) {
            const int r = rows_prev ? L.row4col[k] : k, j = rows_prev ? k : L.col4row[k];
            if (r >= 0 && j >= 0) {
                const double dy = (double)(L.ry[r] - L.cy[j]), dx = (double)(L.rx[r] - L.cx[j]);
                if (sqrt(dy * dy + dx * dx) <= max_distance) partner = rows_prev ? r : j;
            }
        }
        out[k] = partner;
    }
}

// ---- gap closing ----------------------------------------------------------------------------------------------------
// A link of frame f counts when it names a detection of frame f - 1 and f does not open a movie.
__device__ __forceinline__ bool lk_link_valid(int l, int n_prev) { return l >= 0 && l < n_prev; }

// One workgroup per frame f: clears the frame's rows of both outputs and writes has_succ[f, i] = some detection of frame
// f + 1 links to i.  The flags are gathered in LDS, so that every byte of the row is stored once.
__global__ __launch_bounds__(CH_THREADS) void gc_init_kernel(const int *__restrict__ link, const int *__restrict__ count,
                                                              const unsigned char *__restrict__ movie_start, int F, int cap,
                                                              int *__restrict__ gap_partner, int *__restrict__ gap_frames,
                                                              unsigned char *__restrict__ has_succ) {
    __shared__ unsigned char flag[LK_MAX_N];
    const int f = blockIdx.x, tid = threadIdx.x;
    for (int k = tid; k < cap; k += CH_THREADS) {
        flag[k] = 0;
        gap_partner[(int64_t)f * cap + k] = -1;
        gap_frames[(int64_t)f * cap + k] = 0;
    }
    __syncthreads();
    if (f + 1 < F && !(movie_start && movie_start[f + 1])) {
        const int n = lk_clamp_count(count[f], cap), n_next = lk_clamp_count(count[f + 1], cap);
        for (int j = tid; j < n_next; j += CH_THREADS) {
            const int l = link[(int64_t)(f + 1) * cap + j];
            if (lk_link_valid(l, n)) flag[l] = 1;                         // several writers store the same value
        }
    }
    __syncthreads();
    for (int k = tid; k < cap; k += CH_THREADS) has_succ[(int64_t)f * cap + k] = flag[k];
}

// Pass g, workgroup f (one wave): the open ends of frame f - g against the open starts of frame f.  has_succ and gap_frames
// are read and written by this workgroup in the rows f - g and f alone (see the head of the file), hence no __restrict__.
__global__ __launch_bounds__(LK_WAVE) void gc_pass_kernel(const int *__restrict__ coords, const int *__restrict__ count,
                                                          const int *__restrict__ link,
                                                          const unsigned char *__restrict__ movie_start, int cap, int g,
                                                          double max_distance, int *gap_partner, int *gap_frames,
                                                          unsigned char *has_succ) {
    extern __shared__ double lk_lds[];
    const int C = (cap + 7) / 8 * 8;
    const LkLds L = lk_carve(lk_lds, C);
    int *emap = reinterpret_cast<int *>(L.SC + C), *smap = emap + C;      // compacted index -> detection index
    const int f = blockIdx.x, lane = threadIdx.x, f0 = f - g;
    if (f0 < 0) return;
    if (movie_start)
        for (int k = f0 + 1; k <= f; ++k)
            if (movie_start[k]) return;                                   // uniform: every lane reads the same flags
    const int n0 = lk_clamp_count(count[f0], cap), n1 = lk_clamp_count(count[f], cap);
    const int n_before = lk_clamp_count(count[f - 1], cap);              // f >= g >= 2: frame f - 1 exists
    unsigned char *ends = has_succ + (int64_t)f0 * cap;
    int *gp = gap_partner + (int64_t)f * cap, *gf = gap_frames + (int64_t)f * cap;
    const int *lk = link + (int64_t)f * cap;
    const unsigned long long below = (1ull << lane) - 1ull;
    int nE = 0, nS = 0;
    for (int base = 0; base < n0; base += LK_WAVE) {                      // ascending detection index
        const int i = base + lane;
        const bool open = i < n0 && !ends[i];
        const unsigned long long mask = __ballot(open);
        if (open) emap[nE + __popcll(mask & below)] = i;
        nE += __popcll(mask);
    }
    for (int base = 0; base < n1; base += LK_WAVE) {
        const int j = base + lane;
        const bool open = j < n1 && !lk_link_valid(lk[j], n_before) && gf[j] == 0;
        const unsigned long long mask = __ballot(open);
        if (open) smap[nS + __popcll(mask & below)] = j;
        nS += __popcll(mask);
    }
    if (nE == 0 || nS == 0) return;
    __syncthreads();
    const bool rows_end = nE <= nS;                                       // the smaller side plays rows, the ends on equality
    const int nr = rows_end ? nE : nS, nc = rows_end ? nS : nE;
    const int *rmap = rows_end ? emap : smap, *cmap = rows_end ? smap : emap;
    const int *rsrc = coords + (int64_t)(rows_end ? f0 : f) * cap * 2;
    const int *csrc = coords + (int64_t)(rows_end ? f : f0) * cap * 2;
    for (int i = lane; i < nr; i += LK_WAVE) {
        const int d = rmap[i];
        L.ry[i] = rsrc[2 * d];
        L.rx[i] = rsrc[2 * d + 1];
        L.u[i] = 0.0;
        L.col4row[i] = -1;
    }
    for (int j = lane; j < nc; j += LK_WAVE) {
        const int d = cmap[j];
        L.cy[j] = csrc[2 * d];
        L.cx[j] = csrc[2 * d + 1];
        L.v[j] = 0.0;
        L.row4col[j] = -1;
    }
    __syncthreads();
    lk_solve(L, nr, nc, lane);
    for (int k = lane; k < nS; k += LK_WAVE) {                            // solve first, filter afterwards
        const int r = rows_end ? L.row4col[k] : k, j = rows_end ? k : L.col4row[k];
        if (r < 0 || j < 0) continue;
        const double dy = (double)(L.ry[r] - L.cy[j]), dx = (double)(L.rx[r] - L.cx[j]);
        if (!(sqrt(dy * dy + dx * dx) <= max_distance)) continue;         // a dropped pair leaves both ends open
        const int e = emap[rows_end ? r : j], s = smap[k];
        gp[s] = e;
        gf[s] = g;
        ends[e] = 1;
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

// lk_chain_kernel with gap links: ids of the last max_gap + 2 frames in an LDS ring (slot f % ring), lengths by one atomic
// per detection on the cleared array.
__global__ __launch_bounds__(CH_THREADS) void lk_chain_gaps_kernel(const int *__restrict__ link,
                                                                    const int *__restrict__ gap_partner,
                                                                    const int *__restrict__ gap_frames,
                                                                    const int *__restrict__ count,
                                                                    const unsigned char *__restrict__ movie_start, int F,
                                                                    int cap, int max_gap, int *__restrict__ ids,
                                                                    int *__restrict__ lengths, int *__restrict__ n_tracks) {
    extern __shared__ int ch_lds[];                                       // [ring][cap] ids
    __shared__ int wave_total[2][CH_THREADS / LK_WAVE];
    const int ring = max_gap + 2;
    const int tid = threadIdx.x, lane = tid & (LK_WAVE - 1), wave = tid / LK_WAVE;
    int next_id = 0, parity = 0;
    for (int f = 0; f < F; ++f) {
        const int n = lk_clamp_count(count[f], cap);
        const int n_prev = f > 0 ? lk_clamp_count(count[f - 1], cap) : 0;
        const bool fresh = f == 0 || (movie_start && movie_start[f]);
        int *id_cur = ch_lds + (f % ring) * cap;
        for (int base = 0; base < n; base += CH_THREADS) {
            const int j = base + tid;
            const bool valid = j < n;
            int src_frame = -1, src = -1;                                 // where the id comes from
            if (valid && !fresh) {
                const int l = link[(int64_t)f * cap + j];
                if (lk_link_valid(l, n_prev)) {
                    src_frame = f - 1;
                    src = l;
                } else {
                    const int g = gap_frames[(int64_t)f * cap + j];
                    if (g >= 2 && g <= max_gap + 1 && f - g >= 0) {       // the ring still holds frame f - g
                        const int p = gap_partner[(int64_t)f * cap + j];
                        if (lk_link_valid(p, lk_clamp_count(count[f - g], cap))) {
                            src_frame = f - g;
                            src = p;
                        }
                    }
                }
            }
            const bool is_new = valid && src < 0;
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
                const int id = is_new ? next_id + off : ch_lds[(src_frame % ring) * cap + src];
                id_cur[j] = id;
                ids[(int64_t)f * cap + j] = id;
                atomicAdd(&lengths[id], 1);
            }
            next_id += total;
        }
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

extern "C" int mivit_close_gaps(const int *coords, const int *count, const int *link, const unsigned char *movie_start, int F,
                                int cap, int max_gap, double max_distance, int *gap_partner, int *gap_frames,
                                unsigned char *workspace, size_t workspace_bytes, void *stream) {
    MIVIT_CHECK(F >= 0, "close_gaps: F = %d < 0", F);
    MIVIT_CHECK(cap >= 1 && cap <= LK_MAX_N, "close_gaps: capacity of %d detections per frame (1 .. %d)", cap, LK_MAX_N);
    MIVIT_CHECK(max_gap >= 1 && max_gap <= LK_MAX_GAP, "close_gaps: max_gap = %d (1 .. %d)", max_gap, LK_MAX_GAP);
    MIVIT_CHECK(!(max_distance != max_distance), "close_gaps: max_distance is NaN");
    if (F == 0) return 0;
    MIVIT_CHECK(coords && count && link && gap_partner && gap_frames && workspace, "close_gaps: null pointer");
    MIVIT_CHECK(workspace_bytes >= (size_t)F * cap, "close_gaps: workspace of %zu bytes, %zu needed", workspace_bytes,
                (size_t)F * cap);
    static_assert(gc_lds_bytes(LK_MAX_N) <= 64 * 1024, "the gap kernel's LDS plan exceeds the default dynamic limit");
    hipStream_t s = static_cast<hipStream_t>(stream);
    prof_set_tag(MIVIT_PROF_OP);
    hipLaunchKernelGGL(gc_init_kernel, dim3((unsigned)F), dim3(CH_THREADS), 0, s, link, count, movie_start, F, cap, gap_partner,
                       gap_frames, workspace);
    MIVIT_LAUNCH_CHECK();
    for (int g = 2; g <= max_gap + 1 && g < F; ++g) {                     // with g >= F no pair of frames is g apart
        hipLaunchKernelGGL(gc_pass_kernel, dim3((unsigned)F), dim3(LK_WAVE), gc_lds_bytes(cap), s, coords, count, link,
                           movie_start, cap, g, max_distance, gap_partner, gap_frames, workspace);
        MIVIT_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mivit_chain_tracks_gaps(const int *link, const int *gap_partner, const int *gap_frames, const int *count,
                                       const unsigned char *movie_start, int F, int cap, int max_gap, int *ids, int *lengths,
                                       int *n_tracks, void *stream) {
    MIVIT_CHECK(F >= 0, "chain_tracks_gaps: F = %d < 0", F);
    MIVIT_CHECK(cap >= 1 && cap <= LK_MAX_N, "chain_tracks_gaps: capacity of %d detections per frame (1 .. %d)", cap, LK_MAX_N);
    MIVIT_CHECK(max_gap >= 1 && max_gap <= LK_MAX_GAP, "chain_tracks_gaps: max_gap = %d (1 .. %d)", max_gap, LK_MAX_GAP);
    MIVIT_CHECK(n_tracks, "chain_tracks_gaps: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (F == 0) {
        MIVIT_HIP(hipMemsetAsync(n_tracks, 0, sizeof(int), s));
        return 0;
    }
    MIVIT_CHECK(link && gap_partner && gap_frames && count && ids && lengths, "chain_tracks_gaps: null pointer");
    prof_set_tag(MIVIT_PROF_OP);
    MIVIT_HIP(hipMemsetAsync(lengths, 0, (size_t)F * cap * sizeof(int), s));
    hipLaunchKernelGGL(lk_chain_gaps_kernel, dim3(1), dim3(CH_THREADS), (size_t)(max_gap + 2) * cap * sizeof(int), s, link,
                       gap_partner, gap_frames, count, movie_start, F, cap, max_gap, ids, lengths, n_tracks);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
