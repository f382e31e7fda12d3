// Confined diffusion on filament geometries: 1-D displacements along a polyline become 2-D positions (the reference's
// Geometry.map_displacements, Experiments/mitochondria_simulation/mitochnodria.py:339-378, with get_edge_at_length, :231-264, and
// Edge.get_position_at_distance, :87-102).  helpers/geometry._map_host restates the same arithmetic in numpy; in both modes
// the two are bitwise equal, since every operation is a single IEEE fp64 add, subtract, multiply, divide, compare or fmod.
//
// mivit_map_displacements, one launch: one workgroup of 256 threads per particle.  The particle's polyline (vertices and edge
// lengths, both from the host: no device sqrt) is staged in LDS once.  The T steps go through LDS in chunks of GEOM_CHUNK_T
// doubles: all threads load a chunk of disp, coalesced; ONE thread walks it in ascending t, carrying the arc position s from
// chunk to chunk and overwriting d[t] with s after step t; after a barrier all threads look their strided t up (sequential
// subtraction of the edge lengths, the earlier edge wins at a vertex, "no edge found" gives the last vertex) and store pos, arc
// and edge, coalesced.  The walk is a dependent chain whose rounding depends on the order, so it is not scanned in parallel: a
// scan of clamp-add maps is exact in real arithmetic only.  No limit on T.
//
//   clamp(m):  m = (L < m) ? L : m;  m = (m > 0) ? m : 0          Python's max(0, min(m, L)) for every input, NaN -> 0
//   mode 0 (clamp, the reference):  s = clamp(s0);  s = clamp(s + d[t])
//   mode 1 (reflect):  fold(m): P = 2 L; m = fmod(m, P); if (m < 0) m = m + P; if (m > L) m = P - m; m = clamp(m)
//                      s = fold(s0);  s = fold(s + d[t])          per step on the position itself, not on the free sum
//
// s always ends in [0, L], geom_of and vert_offsets are clamped before use and at most GEOM_MAX_EDGES edges are staged, so
// nothing read from memory can address out of bounds.  No atomics; a particle's result depends on its own row only.
//
// No contraction into FMA, as in diffusion.hip and fbm.hip.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int GEOM_THREADS = 256;
constexpr int GEOM_CHUNK_T = 2048;    // steps per pass through LDS (ops.GEOM_CHUNK_T): 16 KiB
constexpr int GEOM_MAX_EDGES = 512;   // edges of one polyline (ops.GEOM_MAX_EDGES): 513 vertices + 512 lengths, 12 KiB

__device__ __forceinline__ double geom_clamp(double m, double hi) {
    m = (hi < m) ? hi : m;
    m = (m > 0.0) ? m : 0.0;
    return m;
}

template <int MODE>
__device__ __forceinline__ double geom_bound(double m, double L, double P) {
    if (MODE == 1) {
        m = fmod(m, P);
        if (m < 0.0) m = m + P;
        if (m > L) m = P - m;
    }
    return geom_clamp(m, L);
}

template <int MODE>
__global__ __launch_bounds__(GEOM_THREADS) void map_displacements_kernel(
    const double *__restrict__ disp, const double *__restrict__ s0, const int *__restrict__ geom_of,
    const double *__restrict__ verts, const double *__restrict__ lengths, const int *__restrict__ vert_offsets,
    const double *__restrict__ totals, int T, int G, int V, double *__restrict__ pos, double *__restrict__ arc,
    int *__restrict__ edge) {
    __shared__ double vx[2 * (GEOM_MAX_EDGES + 1)];
    __shared__ double len[GEOM_MAX_EDGES];
    __shared__ double chunk[GEOM_CHUNK_T];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x;
    int g = geom_of[n];
    g = g < 0 ? 0 : (g >= G ? G - 1 : g);                                 // never read outside totals / vert_offsets
    int v0 = vert_offsets[g], v1 = vert_offsets[g + 1];
    v0 = v0 < 0 ? 0 : (v0 > V - 2 ? V - 2 : v0);                          // V >= 2: at least one edge inside verts, whatever
    v1 = v1 < v0 + 2 ? v0 + 2 : (v1 > V ? V : v1);                        // vert_offsets holds
    const int E = (v1 - v0 - 1 > GEOM_MAX_EDGES) ? GEOM_MAX_EDGES : v1 - v0 - 1;
    const double L = totals[g], P = 2.0 * L;
    for (int i = tid; i < 2 * (E + 1); i += GEOM_THREADS) vx[i] = verts[(int64_t)v0 * 2 + i];
    for (int i = tid; i < E; i += GEOM_THREADS) len[i] = lengths[v0 + i];
    double s = 0.0;
    if (tid == 0) s = geom_bound<MODE>(s0[n], L, P);
    const int64_t row = n * (int64_t)T;
    for (int64_t c0 = 0; c0 < T; c0 += GEOM_CHUNK_T) {
        const int m = (T - c0 < GEOM_CHUNK_T) ? (int)(T - c0) : GEOM_CHUNK_T;
        for (int i = tid; i < m; i += GEOM_THREADS) chunk[i] = disp[row + c0 + i];
        __syncthreads();                                                  // the chunk (and, the first time, the polyline) is staged
        if (tid == 0) {
#pragma unroll 8
            for (int i = 0; i < m; ++i) {
                s = geom_bound<MODE>(s + chunk[i], L, P);
                chunk[i] = s;
            }
        }
        __syncthreads();                                                  // chunk holds arc
        for (int i = tid; i < m; i += GEOM_THREADS) {
            const double a = chunk[i];
            double rem = a;
            int e = 0;
            for (; e < E; ++e) {
                const double le = len[e];
                if (rem <= le) break;                                     // at a vertex the earlier edge wins
                rem = rem - le;
            }
            double p0, p1;
            if (e < E) {
                const double le = len[e];
                const double f = geom_clamp(rem, le) / le;
                p0 = vx[2 * e] + f * (vx[2 * e + 2] - vx[2 * e]);
                p1 = vx[2 * e + 1] + f * (vx[2 * e + 3] - vx[2 * e + 1]);
            } else {                                                      // the remainder is a few ulps above the last length
                e = E - 1;
                p0 = vx[2 * E];
                p1 = vx[2 * E + 1];
            }
            const int64_t o = row + c0 + i;
            pos[2 * o] = p0;
            pos[2 * o + 1] = p1;
            if (arc) arc[o] = a;
            if (edge) edge[o] = e;
        }
        __syncthreads();                                                  // everyone has read the chunk before the next load
    }
}

}  // namespace

extern "C" int mivit_map_displacements(const double *disp, const double *s0, const int *geom_of, const double *verts,
                                       const double *lengths, const int *vert_offsets, const double *totals, int N, int T, int G,
                                       int V, int mode, double *pos, double *arc, int *edge, void *stream) {
    MIVIT_CHECK(N >= 0 && T >= 0 && G >= 0 && V >= 0, "map_displacements: N = %d, T = %d, G = %d, V = %d: negative size", N, T, G, V);
    MIVIT_CHECK(mode == 0 || mode == 1, "map_displacements: mode = %d, 0 (clamp) and 1 (reflect) are supported", mode);
    if (N == 0 || T == 0) return 0;
    MIVIT_CHECK(G >= 1, "map_displacements: no geometry (G = 0) for %d particles", N);
    MIVIT_CHECK(V >= 2 * (int64_t)G, "map_displacements: V = %d vertices cannot give each of G = %d geometries an edge", V, G);
    // vert_offsets lives on the device; what the sizes alone prove is rejected here, the rest in ops.map_displacements
    MIVIT_CHECK((int64_t)V - G <= (int64_t)G * GEOM_MAX_EDGES,
                "map_displacements: V = %d vertices in G = %d geometries: a geometry has more than %d edges (the polyline lives in LDS)",
                V, G, GEOM_MAX_EDGES);
    MIVIT_CHECK(disp && s0 && geom_of && verts && lengths && vert_offsets && totals && pos, "map_displacements: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    prof_set_tag(MIVIT_PROF_OP);
    if (mode == 0)
        hipLaunchKernelGGL(map_displacements_kernel<0>, dim3((unsigned)N), dim3(GEOM_THREADS), 0, s, disp, s0, geom_of, verts,
                           lengths, vert_offsets, totals, T, G, V, pos, arc, edge);
    else
        hipLaunchKernelGGL(map_displacements_kernel<1>, dim3((unsigned)N), dim3(GEOM_THREADS), 0, s, disp, s0, geom_of, verts,
                           lengths, vert_offsets, totals, T, G, V, pos, arc, edge);
    MIVIT_LAUNCH_CHECK();
    return 0;
}
