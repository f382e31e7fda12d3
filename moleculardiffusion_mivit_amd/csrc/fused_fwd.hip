// Fused forward kernels of the post-norm encoder layer, 16-bit modes, for two layer widths chosen PER TRANSLATION UNIT
// (elem.h): E = 128 / F = 256 / head dim 32 (the PSFNoise 32x64x64 configuration) and, under -DMIVIT_WIDTH64, the
// reference's shipped E = 64 / F = 128 / head dim 16 (Experiments/Framerate/trainSettingsFramerate.py:42-47); 4 heads both.
// Reference helpers/models.py:97-108 TransformerEncoderLayerWithSkip, :33-59 attention, :72-77 feed-forward:
//
//   attn_block_fwd :  n1 = LNhat( x + out_proj(attention(q_proj x, k_proj x, v_proj x)) )      one wave per SEQUENCE
//   mlp_block_fwd  :  n2 = LNhat( x1 + fc2(act(fc1 x1)) )                                      one wave per 32 ROWS
//
// Both read their input ONCE and write the normalised output ONCE (+ the attention context, which the out-projection's
// weight gradient needs).  Everything between lives in registers:
//   * the layer weights sit in LDS for the lifetime of a persistent workgroup (one per CU, 8 waves), as MFMA operand
//     images with a conflict-free row pitch;
//   * a product is computed TRANSPOSED (weights as the MFMA row operand, activation rows as the column operand):
//     the accumulator of Y^T (lane = activation row, registers = 4 consecutive output features) IS the column operand
//     of the next product, once the next weight image is stored with the matching permutation of its contraction
//     index (inside each block of 32: slot 8g+j <- k = 4g+j, slot 8g+4+j <- k = 16+4g+j).  QKV -> scores -> softmax
//     -> PV -> out-projection -> residual -> LayerNorm, and FC1 -> activation -> FC2 -> residual -> LayerNorm, never
//     touch LDS or HBM in between; V is computed un-transposed so that its accumulator (lane = head feature,
//     registers = keys) is the operand of P V with the same key permutation as the probabilities.
//   * LayerNorm outputs are stored NORMALISED (xhat = (z - mean) * rstd, bf16) with rstd per row; the consumer applies
//     the affine (gamma * xhat + beta) while loading.  The backward needs exactly xhat and rstd, so neither the
//     pre-norm sum nor the mean is kept.
// Optional outputs (x = gamma * xhat + beta, the pre-norm sum z, q|k|v, h) serve the unfused backward kernels.
#include "common.h"
#include "stream_prims.h"
#include <stdlib.h>
#include <algorithm>
#include "elem.h"          // element type of this translation unit (bf16, or f16 under -DMIVIT_ELEM_F16): after every other include

#define RC(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

namespace {

#ifdef MIVIT_WIDTH64
constexpr int E = 64, F = 128, H = 4, DH = 16;
constexpr int LDE = E + 16;          // LDS row pitch (elements) of a [*, 64] operand image: 160 B = 10 x 16 B
constexpr int LDF = F + 16;          // ... of a [*, 128] image: 288 B = 18 x 16 B   (pitches of 2, 6, 10, 14 mod 16 units: conflict-free b128)
constexpr float QSCALE = 0.25f * 1.4426950408889634f;                     // 1/sqrt(16) * log2(e), folded into the q projection
#else
constexpr int E = 128, F = 256, H = 4, DH = 32;
constexpr int LDE = E + 16;          // LDS row pitch (elements) of a [*, 128] operand image: 288 B = 18 x 16 B
constexpr int LDF = F + 16;          // ... of a [*, 256] image: 544 B = 34 x 16 B   (pitch = 2 mod 16 units: conflict-free b128)
constexpr float QSCALE = 0.17677669529663687f * 1.4426950408889634f;      // 1/sqrt(32) * log2(e), folded into the q projection
#endif
constexpr int KS = E / 32;           // contraction steps of a projection over the embedding (32 per MFMA)
constexpr int ET = E / 16;           // 16-feature tiles of an embedding row
constexpr int DT = DH / 16;          // 16-feature tiles of a head
constexpr int HB = 32 / DH;          // heads per 32-wide contraction block of the out-projection
constexpr int NWAVES = 8, NTHREADS = NWAVES * 64;

__device__ __forceinline__ bf16x8 pack8(const f32x4 a, const f32x4 b) {
    bf16x8 f;
    f[0] = (__bf16)a[0]; f[1] = (__bf16)a[1]; f[2] = (__bf16)a[2]; f[3] = (__bf16)a[3];
    f[4] = (__bf16)b[0]; f[5] = (__bf16)b[1]; f[6] = (__bf16)b[2]; f[7] = (__bf16)b[3];
    return f;
}
__device__ __forceinline__ float x4_sum(float v) { return rows4_sum(v); }   // across the 4 lane groups (same lane & 15): common.h
__device__ __forceinline__ float x4_max(float v) { return rows4_max(v); }
__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
// (A hand-written v_max3_f32 for the softmax's running maximum -- fmaxf costs a canonicalising v_max_f32 x, x, x per operand in
//  IEEE mode, 216 of them per sequence -- was tried in round 3 and REMOVED: an inline-asm VALU instruction that reads MFMA results
//  is invisible to the compiler's hazard recogniser, no wait states were inserted behind the MFMA, and the maximum was read
//  before the matrix pipe had written it.  The softmax is invariant to the value of the maximum up to rounding, so every
//  tolerance test passed; the bitwise-repeatability and strict-waits tests caught it.)
// the two 8-byte halves of a packed fragment (4 + 4 elements): row stores reuse the registers the MFMA operand was packed
// into instead of converting the same accumulators a second time
__device__ __forceinline__ void store_halves(bf16 *p_lo, bf16 *p_hi, const bf16x8 f) {
    struct H { uint2 lo, hi; };
    const H h = __builtin_bit_cast(H, f);
    *reinterpret_cast<uint2 *>(p_lo) = h.lo;
    *reinterpret_cast<uint2 *>(p_hi) = h.hi;
}
__device__ __forceinline__ void store_lo(bf16 *p_lo, const bf16x8 f) {
    struct H { uint2 lo, hi; };
    *reinterpret_cast<uint2 *>(p_lo) = __builtin_bit_cast(H, f).lo;
}
__device__ __forceinline__ bf16x8 lds_frag(const bf16 *p) { return *reinterpret_cast<const bf16x8 *>(p); }

// 4 consecutive bf16 -> fp32 / fp32 -> 4 consecutive bf16 (8-byte global accesses)
__device__ __forceinline__ f32x4 load4_bf16(const bf16 *p) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    return f32x4{elem_lo(v.x), elem_hi(v.x), elem_lo(v.y), elem_hi(v.y)};
}
__device__ __forceinline__ void store4_bf16(bf16 *p, const f32x4 v) {
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    const bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};      // two v_cvt_pk_bf16_f32
    *reinterpret_cast<bf16x4 *>(p) = o;
}

// ---- rows of one tile / one sequence as a RAW BUFFER (buffer_load / buffer_store with a resource descriptor in SGPRs) ----
// The hardware range check does what per-row branches did: an access at or past `bytes` is dropped (stores) or returns zero
// (loads).  Rows that do not exist (past the end of the sequence / of the last tile) start exactly at `bytes`, so every row access
// is issued unconditionally, with a 32-bit lane offset that is loop-invariant plus an immediate: no 64-bit address arithmetic
// (232 vector instructions per sequence in attn_block_fwd), no exec-mask branches around the stores (~340 scalar instructions), and
// straight-line code the compiler can schedule across and count its vmcnt through.
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t rows_of(const void *first_row_uniform, int bytes) {          // (base must be wave-uniform)
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(first_row_uniform), 0, bytes, 0x00020000);
}
__device__ __forceinline__ void bst4_bf16(rsrc_t r, int off, const f32x4 v) {
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    const bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};      // two v_cvt_pk_bf16_f32
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, o), r, off, 0, 0);
}
__device__ __forceinline__ void bst_halves(rsrc_t r, int off, const bf16x8 f) {          // the two 8-byte halves, 32 bytes apart
    struct H { u32x2_t lo, hi; };
    const H h = __builtin_bit_cast(H, f);
    __builtin_amdgcn_raw_buffer_store_b64(h.lo, r, off, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b64(h.hi, r, off + 32, 0, 0);
}
__device__ __forceinline__ void bst_lo(rsrc_t r, int off, const bf16x8 f) {
    struct H { u32x2_t lo, hi; };
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(H, f).lo, r, off, 0, 0);
}
__device__ __forceinline__ void bst_f32(rsrc_t r, int off, float v) { __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, off, 0, 0); }
__device__ __forceinline__ uint4 bld16(rsrc_t r, int off) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    return make_uint4(v[0], v[1], v[2], v[3]);
}
constexpr int OOB = 0x7ffffff0;          // a lane offset past any descriptor: that lane's access is dropped

// natural [rows][K] bf16 weight block (row pitch ldw elements) -> LDS operand image with pitch LD
// The staging loops issue SU iterations' loads before the first store: with one load -> wait -> store per iteration (what a
// loop with a run-time trip count compiles to) a workgroup spent 24 + 8 + ... serialised L2 round trips on its weights.
constexpr int SU = 8;
template <int K, int LD>
__device__ __forceinline__ void stage_natural(bf16 *img, const bf16 *W, int rows, int tid, int nthr = NTHREADS) {
    const int n = rows * (K / 8);
    for (int i0 = tid; i0 < n; i0 += SU * nthr) {
        uint4 v[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const int i = min(i0 + u * nthr, n - 1), r = i / (K / 8), c = i - r * (K / 8);          // (clamped: always a valid load)
            v[u] = *reinterpret_cast<const uint4 *>(W + (int64_t)r * K + c * 8);
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const int i = i0 + u * nthr, r = i / (K / 8), c = i - r * (K / 8);
            if (i < n) *reinterpret_cast<uint4 *>(img + r * LD + c * 8) = v[u];
        }
    }
}
// the same with the contraction index permuted inside each block of 32 so that the 16-byte chunk g of block p holds
// k = 32p + 4g + {0..3} and k = 32p + 16 + 4g + {0..3}: the operand that meets a packed accumulator pair
template <int K, int LD>
__device__ __forceinline__ void stage_permuted(bf16 *img, const bf16 *W, int rows, int tid, int nthr = NTHREADS) {
    const int n = rows * (K / 8);
    for (int i0 = tid; i0 < n; i0 += SU * nthr) {
        uint2 lo[SU], hi[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const int i = min(i0 + u * nthr, n - 1), r = i / (K / 8), c = i - r * (K / 8), p = c >> 2, g = c & 3;
            lo[u] = *reinterpret_cast<const uint2 *>(W + (int64_t)r * K + 32 * p + 4 * g);
            hi[u] = *reinterpret_cast<const uint2 *>(W + (int64_t)r * K + 32 * p + 16 + 4 * g);
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const int i = i0 + u * nthr, r = i / (K / 8), c = i - r * (K / 8);
            if (i < n) *reinterpret_cast<uint4 *>(img + r * LD + c * 8) = make_uint4(lo[u].x, lo[u].y, hi[u].x, hi[u].y);
        }
    }
}
__device__ __forceinline__ void stage_vec(float *dst, const float *src, int n, float fill, int tid, int nthr = NTHREADS) {
    for (int i = tid; i < n; i += nthr) dst[i] = src ? src[i] : fill;
}

// column-operand fragments of 16 activation rows: lane (row = lane & 15, g) holds k = 32 ks + 8 g + 0..7.
// load_raw issues the KS 16-byte loads (zeros for rows that do not exist); the registers ARE the MFMA operands.
// (off = the lane's row offset inside the descriptor + 16 g)
__device__ __forceinline__ void load_raw(uint4 (&raw)[KS], rsrc_t rows, int off) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) raw[ks] = bld16(rows, off + ks * 64);
}
__device__ __forceinline__ bf16x8 as_frag(const uint4 &u) { return __builtin_bit_cast(bf16x8, u); }
// The producing LayerNorm's affine is FOLDED into the consuming weights while they are staged (once per workgroup):
//   (gamma * n + beta) W^T + b  =  n (W * gamma)^T + (b + W beta)
// so the projections run on the raw normalised rows exactly as loaded -- no per-element affine, no copy.
template <int K, int LD>
__device__ __forceinline__ void stage_folded(bf16 *img, const bf16 *W, int rows, const float *gam, int tid, int nthr = NTHREADS,
                                             int rs_rows = 0, float rs_val = 1.f) {      // rows < rs_rows are scaled by rs_val
    const int n = rows * (K / 8);
    for (int i0 = tid; i0 < n; i0 += SU * nthr) {
        uint4 raw[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const int i = min(i0 + u * nthr, n - 1), r = i / (K / 8), c = i - r * (K / 8);
            raw[u] = *reinterpret_cast<const uint4 *>(W + (int64_t)r * K + c * 8);
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const int i = i0 + u * nthr, r = i / (K / 8), c = i - r * (K / 8);
            if (i < n) {
                const float rsc = r < rs_rows ? rs_val : 1.f;
                const uint32_t w[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
                float v[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[2 * e] = elem_lo(w[e]); v[2 * e + 1] = elem_hi(w[e]); }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= gam[c * 8 + e] * rsc;
                store16(img + r * LD + c * 8, v);
            }
        }
    }
}
// dst[r] = b[r] + sum_k W[r][k] beta[k]   (beta == nullptr: plain copy)
template <int K>
__device__ __forceinline__ void fold_bias(float *dst, const float *b, const bf16 *W, int rows, const float *bet, bool fold, int tid,
                                          int nthr = NTHREADS, int rs_rows = 0, float rs_val = 1.f) {
    for (int r = tid; r < rows; r += nthr) {
        float acc = b ? b[r] : 0.f;
        if (fold) {
#pragma unroll
            for (int c = 0; c < K / 8; ++c) {
                float v[8];
                load16(W + (int64_t)r * K + c * 8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += v[e] * bet[c * 8 + e];
            }
        }
        dst[r] = r < rs_rows ? acc * rs_val : acc;
    }
}
// The residual needs the input rows in the ACCUMULATOR layout (lane = row, registers = 4 consecutive features), the
// fragments hold them in the operand layout.  The matrix pipe transposes for free: n^T tile et = I n^T with a constant
// 0/1 row operand that picks features 16 et .. 16 et + 15 out of the 32-wide block ks = et / 2 (exact: one product per
// output); the affine of the residual is then 4 FMAs per tile.  idfrag(par) is that operand for et of parity par.
__device__ __forceinline__ bf16x8 idfrag(int par, int cq, int g) {
    bf16x8 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (g == 2 * par + (cq >> 3) && j == (cq & 7)) ? (__bf16)1.0f : (__bf16)0.0f;
    return f;
}

// ---- shared epilogue: z^T accumulators (8 feature tiles of one 16-row block, residual included) -> LayerNorm -> stores ----
struct LnOut {
    bf16 *nout; float *rstd;          // normalised output + 1/std per row (always)
    bf16 *xout;                       // optional: gamma * nhat + beta
    bf16 *zout; float *mean;          // optional: pre-norm sum and mean (unfused backward)
};
// the same for `rows` rows starting at `first_row` (wave-uniform), as raw buffers
struct LnDst { rsrc_t n, rstd, x, z, mean; bool hx, hz, hm; };
__device__ __forceinline__ LnDst ln_dst(const LnOut &o, int64_t first_row, int rows) {
    LnDst d;
    d.n = rows_of(o.nout + first_row * E, rows * E * 2);
    d.rstd = rows_of(o.rstd + first_row, rows * 4);
    d.hx = o.xout != nullptr; d.hz = o.zout != nullptr; d.hm = o.mean != nullptr;
    d.x = rows_of(d.hx ? o.xout + first_row * E : nullptr, d.hx ? rows * E * 2 : 0);
    d.z = rows_of(d.hz ? o.zout + first_row * E : nullptr, d.hz ? rows * E * 2 : 0);
    d.mean = rows_of(d.hm ? o.mean + first_row : nullptr, d.hm ? rows * 4 : 0);
    return d;
}
// voe: the lane's byte offset of (its row, feature 4 g) in an [*, E] 16-bit row buffer; vor: its row's offset in a per-row fp32
// buffer for the lanes g == 0, OOB for the others
__device__ __forceinline__ void ln_store(f32x4 (&z)[ET], const LnDst &d, int voe, int vor, const float *gout, const float *bout) {
    float s = 0.f;
#pragma unroll
    for (int et = 0; et < ET; ++et) s += z[et][0] + z[et][1] + z[et][2] + z[et][3];
    const float mu = x4_sum(s) * (1.f / E);
    float q = 0.f;
#pragma unroll
    for (int et = 0; et < ET; ++et)
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float dd = z[et][j] - mu; q += dd * dd; }
    const float rs = rsqrtf(x4_sum(q) * (1.f / E) + 1e-5f);
#pragma unroll
    for (int et = 0; et < ET; ++et) {
        const int c = 16 * et;          // (+ 4 g: in voe)
        if (d.hz) bst4_bf16(d.z, voe + 2 * c, z[et]);
        f32x4 nh;
#pragma unroll
        for (int j = 0; j < 4; ++j) nh[j] = (z[et][j] - mu) * rs;
        bst4_bf16(d.n, voe + 2 * c, nh);
        if (d.hx) {
            const int cg = c + (voe & 31) / 2;          // = 16 et + 4 g  (rows are multiples of 32 bytes)
            bst4_bf16(d.x, voe + 2 * c, nh * ld4(gout + cg) + ld4(bout + cg));
        }
    }
    bst_f32(d.rstd, vor, rs);
    if (d.hm) bst_f32(d.mean, vor, mu);
}

// ================================================================================================================
// MLP block
// ================================================================================================================
struct MlpFwdArgs {
    const bf16 *nin; const float *gin, *bin;      // input rows [M, E] (normalised; affine gin/bin, or null = identity)
    const bf16 *W1; const float *b1;              // fc1 [F, E] bf16 copy, bias fp32
    const bf16 *W2; const float *b2;              // fc2 [E, F]
    const float *gout, *bout;                     // this sub-layer's LayerNorm affine (only for xout)
    int M, act;
    LnOut o;
    bf16 *hout, *uout;                            // optional: post-activation h [M, F] and pre-activation (GELU backward)
};

constexpr int MLP_LDS_W1 = F * LDE * 2, MLP_LDS_W2 = E * LDF * 2;
constexpr int MLP_VEC = E * 5 + F;               // gin, bin, b2, gout, bout [E] + b1 [F]
constexpr int MLP_LDS = MLP_LDS_W1 + MLP_LDS_W2 + MLP_VEC * 4;
static_assert(MLP_LDS <= 160 * 1024, "LDS budget");

// (Width 64: two workgroups per CU fit -- 37 KB of weight images, <= 128 registers -- and were measured at the Framerate shape:
//  attn_block_fwd 32.1 / 30.8 us, mlp_block_fwd 17.7 / 19.5 us with grids of 512 / 256: no difference, one per CU kept.)
template <int NR, int ACT, bool EXTRAS, int NWV = NWAVES>      // EXTRAS: the optional h / pre-activation outputs are compiled in; NWV waves per workgroup
__global__ __launch_bounds__(NWV * 64) void mlp_block_fwd_kernel(const MlpFwdArgs a) {
    constexpr int NTH = NWV * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16 *W1i = reinterpret_cast<bf16 *>(smem);
    bf16 *W2i = reinterpret_cast<bf16 *>(smem + MLP_LDS_W1);
    float *vec = reinterpret_cast<float *>(smem + MLP_LDS_W1 + MLP_LDS_W2);
    float *gin = vec, *bin = vec + E, *b2 = vec + 2 * E, *gout = vec + 3 * E, *bout = vec + 4 * E, *b1 = vec + 5 * E;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, cq = lane & 15;
    const bool affine_in = a.gin != nullptr;
    stage_vec(gin, a.gin, E, 1.f, tid, NTH); stage_vec(bin, a.bin, E, 0.f, tid, NTH);
    stage_vec(gout, a.gout, E, 1.f, tid, NTH); stage_vec(bout, a.bout, E, 0.f, tid, NTH);
    __syncthreads();
    if (affine_in) stage_folded<E, LDE>(W1i, a.W1, F, gin, tid, NTH); else stage_natural<E, LDE>(W1i, a.W1, F, tid, NTH);
    stage_permuted<F, LDF>(W2i, a.W2, E, tid, NTH);
    fold_bias<E>(b1, a.b1, a.W1, F, bin, affine_in, tid, NTH);
    for (int i = tid; i < E; i += NTH) b2[i] = a.b2[i] + bin[i];          // fc2 bias + the residual's beta
    __syncthreads();
    const int ntiles = (a.M + 16 * NR - 1) / (16 * NR);
    const bf16x8 id0 = idfrag(0, cq, g), id1 = idfrag(1, cq, g);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int tile = blockIdx.x * NWV + __builtin_amdgcn_readfirstlane(wave);          // (scalar: the tile's buffer descriptors live in SGPRs)
    const int tstride = gridDim.x * NWV;
    // lane offsets inside a tile's row buffers (loop-invariant): [*, E] 16-bit rows for loads (+ 16 g) and stores (+ 8 g), [*, F]
    // rows, per-row fp32 values (lanes g == 0)
    int vo_l[NR], vo_e[NR], vo_f[NR], vo_r[NR];
#pragma unroll
    for (int rb = 0; rb < NR; ++rb) {
        vo_l[rb] = (rb * 16 + cq) * E * 2 + 16 * g; vo_e[rb] = (rb * 16 + cq) * E * 2 + 8 * g;
        vo_f[rb] = (rb * 16 + cq) * F * 2 + 8 * g;  vo_r[rb] = g == 0 ? (rb * 16 + cq) * 4 : OOB;
    }
    auto rows_in = [&](int t) { return min(16 * NR, a.M - t * 16 * NR); };          // (valid rows of tile t)
    uint4 nx[NR][KS];
    if (tile < ntiles) {
        const rsrc_t rin = rows_of(a.nin + (int64_t)tile * 16 * NR * E, rows_in(tile) * E * 2);
#pragma unroll
        for (int rb = 0; rb < NR; ++rb) load_raw(nx[rb], rin, vo_l[rb]);
    }
    for (; tile < ntiles; tile += tstride) {
        const int64_t row0 = (int64_t)tile * 16 * NR;
        bf16x8 xf[NR][KS];
#pragma unroll
        for (int rb = 0; rb < NR; ++rb)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) xf[rb][ks] = as_frag(nx[rb][ks]);
        {                                        // next tile's rows: in flight while this one computes (unconditional --
            const int nxt = min(tile + tstride, ntiles - 1);          // a clamped re-read on the last round -- so the
            const rsrc_t rin = rows_of(a.nin + (int64_t)nxt * 16 * NR * E, rows_in(nxt) * E * 2);      // registers are dead until here)
#pragma unroll
            for (int rb = 0; rb < NR; ++rb) load_raw(nx[rb], rin, vo_l[rb]);
        }
        const LnDst dst = ln_dst(a.o, row0, rows_in(tile));
        const bool has_u = EXTRAS && a.uout != nullptr, has_h = EXTRAS && a.hout != nullptr;
        const rsrc_t ru = rows_of(has_u ? a.uout + row0 * F : nullptr, has_u ? rows_in(tile) * F * 2 : 0);
        const rsrc_t rh = rows_of(has_h ? a.hout + row0 * F : nullptr, has_h ? rows_in(tile) * F * 2 : 0);
        f32x4 fa[ET][NR];
#pragma unroll
        for (int et = 0; et < ET; ++et) {
            const f32x4 bv = ld4(b2 + 16 * et + 4 * g), gv = ld4(gin + 16 * et + 4 * g);
#pragma unroll
            for (int rb = 0; rb < NR; ++rb) fa[et][rb] = bv + gv * mma((et & 1) ? id1 : id0, xf[rb][et >> 1], zero);   // bias + residual
        }
#ifndef MIVIT_MLP_P_UNROLL          // (A/B, scripts/ab_rebuild.sh, us per layer / ms per step: 1 -> 94.1 / 0.499, 2 -> 93.0 / 0.498, 4 -> 102.3 / 0.527, 8 -> 97.3 / 0.540)
#define MIVIT_MLP_P_UNROLL 2
#endif
#pragma unroll MIVIT_MLP_P_UNROLL
        for (int p = 0; p < F / 32; ++p) {
            // h^T for hidden units 32p .. 32p+31 (two feature tiles), all NR row blocks
            f32x4 ha[2][NR];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f32x4 bv = ld4(b1 + 32 * p + 16 * t + 4 * g);
#pragma unroll
                for (int rb = 0; rb < NR; ++rb) ha[t][rb] = bv;
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const bf16x8 w = lds_frag(W1i + (32 * p + 16 * t + cq) * LDE + ks * 32 + 8 * g);
#pragma unroll
                    for (int rb = 0; rb < NR; ++rb) ha[t][rb] = mma(w, xf[rb][ks], ha[t][rb]);
                }
            bf16x8 hf[NR];
#pragma unroll
            for (int rb = 0; rb < NR; ++rb) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (has_u) bst4_bf16(ru, vo_f[rb] + (32 * p + 16 * t) * 2, ha[t][rb]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) ha[t][rb][j] = act_fwd(ACT, ha[t][rb][j]);
                    if (has_h) bst4_bf16(rh, vo_f[rb] + (32 * p + 16 * t) * 2, ha[t][rb]);
                }
                hf[rb] = pack8(ha[0][rb], ha[1][rb]);
            }
            // f^T += W2[:, block p (permuted)] h^T
#pragma unroll
            for (int et = 0; et < ET; ++et) {
                const bf16x8 w = lds_frag(W2i + (16 * et + cq) * LDF + p * 32 + 8 * g);
#pragma unroll
                for (int rb = 0; rb < NR; ++rb) fa[et][rb] = mma(w, hf[rb], fa[et][rb]);
            }
        }
#pragma unroll
        for (int rb = 0; rb < NR; ++rb) {
            f32x4 z[ET];
#pragma unroll
            for (int et = 0; et < ET; ++et) z[et] = fa[et][rb];
            ln_store(z, dst, vo_e[rb], vo_r[rb], gout, bout);
        }
    }
}

// ================================================================================================================
// attention block
// ================================================================================================================
struct AttnFwdArgs {
    const bf16 *nin; const float *gin, *bin;      // input tokens [B*S, E]
    const bf16 *Wqkv; const float *bqkv;          // [3E, E] (q | k | v rows), [3E]
    const bf16 *Wo; const float *bo;              // [E, E]
    const float *gout, *bout;
    int B, S;
    bf16 *ctx;                                    // [B*S, E] attention output before the out-projection (kept: dW_o needs it)
    LnOut o;
    bf16 *qkvout;                                 // optional [B*S, 3E] (unfused attention backward)
};

constexpr int ATT_LDS_WQKV = 3 * E * LDE * 2, ATT_LDS_WO = E * LDE * 2;
constexpr int ATT_VEC = E * 5 + 3 * E;           // gin, bin, bo, gout, bout + bqkv
constexpr int ATT_LDS = ATT_LDS_WQKV + ATT_LDS_WO + ATT_VEC * 4;
static_assert(ATT_LDS <= 160 * 1024, "LDS budget");

// NT row tiles per sequence (S <= 16 NT); EXTRAS: the optional q|k|v output is compiled in; NW waves per workgroup
// (one workgroup per CU: 8 waves share the register file two per SIMD, 4 waves own a whole SIMD's 512 registers each)
// Q1: the QUERY side for row tile 0 only (the last layer under the regression-token readout: the head reads row 0 of a sequence).
// k and v are projected and stored for every row; q, scores / softmax / P V, out-projection, residual and LayerNorm run for the
// first 16 rows -- the same MFMAs on the same operands as in the full kernel, so those rows are bitwise the full kernel's.  Of the
// rows behind them q, ctx, z and rstd are NOT written, the normalised output is written as ZEROS when the q|k|v store is on (a
// backward follows, and its feed-forward block reads every row) and not at all otherwise.
template <int NT, bool EXTRAS, int NW, bool Q1 = false>
__global__ __launch_bounds__(NW * 64) void attn_block_fwd_kernel(const AttnFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NP = (NT + 1) / 2;
    constexpr int NQ = Q1 ? 1 : NT;                  // query row tiles
    bf16 *Wq = reinterpret_cast<bf16 *>(smem);
    bf16 *Wo = reinterpret_cast<bf16 *>(smem + ATT_LDS_WQKV);
    float *vec = reinterpret_cast<float *>(smem + ATT_LDS_WQKV + ATT_LDS_WO);
    float *gin = vec, *bin = vec + E, *bo = vec + 2 * E, *gout = vec + 3 * E, *bout = vec + 4 * E, *bqkv = vec + 5 * E;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, cq = lane & 15;
    const bool affine_in = a.gin != nullptr;
    stage_vec(gin, a.gin, E, 1.f, tid, NW * 64); stage_vec(bin, a.bin, E, 0.f, tid, NW * 64);
    stage_vec(gout, a.gout, E, 1.f, tid, NW * 64); stage_vec(bout, a.bout, E, 0.f, tid, NW * 64);
    __syncthreads();
    // q rows carry 1/sqrt(head dim) * log2(e): the scores come out of the MFMA ready for exp2
    stage_folded<E, LDE>(Wq, a.Wqkv, 3 * E, gin, tid, NW * 64, E, QSCALE);
    stage_permuted<E, LDE>(Wo, a.Wo, E, tid, NW * 64);
    fold_bias<E>(bqkv, a.bqkv, a.Wqkv, 3 * E, bin, affine_in, tid, NW * 64, E, QSCALE);
    for (int i = tid; i < E; i += NW * 64) bo[i] = a.bo[i] + bin[i];          // out-projection bias + the residual's beta
    __syncthreads();
    const int S = a.S;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    const bf16x8 id0 = idfrag(0, cq, g), id1 = idfrag(1, cq, g);
    const int bstride = gridDim.x * NW;
    int b = blockIdx.x * NW + __builtin_amdgcn_readfirstlane(wave);          // (scalar: a sequence's buffer descriptors live in SGPRs)
    // lane offsets inside a sequence's row buffers (loop-invariant): [S, E] rows for loads (+ 16 g) and stores (+ 8 g), [S, 3E]
    // rows of the q|k|v output, per-row fp32 values (lanes g == 0)
    int vo_l[NT], vo_e[NT], vo_q[NT], vo_r[NT];
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) {
        vo_l[rt] = (rt * 16 + cq) * E * 2 + 16 * g; vo_e[rt] = (rt * 16 + cq) * E * 2 + 8 * g;
        vo_q[rt] = (rt * 16 + cq) * 3 * E * 2 + 8 * g; vo_r[rt] = g == 0 ? (rt * 16 + cq) * 4 : OOB;
    }
    // Next sequence's rows: requested after the attention phase (into the registers the input fragments are read from: dead by
    // then), in flight under the out-projection and the epilogue.
    // (Round 3 built and measured a WRITTEN-OUT form -- inline-asm loads at the top of the iteration, before the iteration's row
    //  stores, and a counted `vmcnt(min(63, stores per iteration))` at the top of the next one -- on the theory that the compiler's
    //  vmcnt(0) in front of the first use drains ~50-170 store acknowledgements per iteration.  It does drain them, and it does not
    //  matter: with the q|k|v store the written-out form was SLOWER at every shape (33 tokens: not applicable, see below; 31
    //  tokens: 256 against 245 us at four waves, 311 against 284 at eight; 16 tokens: 143 against 132), without it within noise
    //  except 31 tokens at four waves (155 against 169); width 64: noise.  It also needed a build-time ISA rule of its own: at three
    //  and four row tiles the allocator parks the asm destinations in accumulation registers right behind the statement -- a copy
    //  of registers the memory system has not written yet.  Removed; scripts/ab_asm_pf.sh and DESIGN.md section 4c keep the numbers.)
    uint4 nxc[NT][KS];
    auto request = [&](int seq) {
        const rsrc_t rin = rows_of(a.nin + (int64_t)seq * S * E, S * E * 2);
#pragma unroll
        for (int rt = 0; rt < NT; ++rt) load_raw(nxc[rt], rin, vo_l[rt]);
    };
    if (b < a.B) request(b);
    for (; b < a.B; b += bstride) {
        const int64_t base = (int64_t)b * S;
        const rsrc_t rctx = rows_of(a.ctx + base * E, S * E * 2);
        const bool has_qkv = EXTRAS && a.qkvout != nullptr;          // (the launcher picks EXTRAS exactly then; a null pointer: everything dropped)
        const rsrc_t rqkv = rows_of(has_qkv ? a.qkvout + base * 3 * E : nullptr, has_qkv ? S * 3 * E * 2 : 0);
        const LnDst dst = ln_dst(a.o, base, S);
        bf16x8 xf[NT][KS];
#pragma unroll
        for (int rt = 0; rt < NT; ++rt)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) xf[rt][ks] = as_frag(nxc[rt][ks]);
        bf16x8 cf[KS][NT];                           // context, as the column operand of the out-projection: one fragment per
        f32x4 ot_even[NT];                           // 32 features = one head (head dim 32) or two (head dim 16: the even head waits here)
        // Weight fragments of a projection block (q, k or v of one head: KS x DT reads of 1 KB) are requested ONE BLOCK AHEAD, as a
        // batch, into the other of two register sets: written as "read a fragment, use it" the compiler keeps each ds_read_b128
        // next to its three MFMAs and waits for it (`L2 w M6` through the whole phase: one LDS round trip per 48-96 MFMA cycles,
        // with one wave per SIMD nobody to cover it -- 220 such reads per sequence).  The accumulators start from the inline
        // constant 0 and the bias is added in the epilogue (as the C operand it cost four register copies per tile and a wait
        // for its own LDS read in front of the first MFMA).  The v^T product for the q|k|v store reuses the v block's fragments.
        constexpr bool WIDE = NW == 4 || E == 64;          // (two waves per SIMD at width 128: 256 registers, the old per-fragment form)
        bf16x8 wb[2][KS][DT];
        auto request_w = [&](int buf, int rowbase) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) wb[buf][ks][dt] = lds_frag(Wq + (rowbase + 16 * dt + cq) * LDE + ks * 32 + 8 * g);
        };
        int cur = 0;
        if constexpr (WIDE) request_w(0, 0);         // q of head 0
#pragma unroll
        for (int h = 0; h < H; ++h) {
            bf16x8 qf[NT], kf[NT], vr[NP][DT];
            if constexpr (WIDE) {
                // ---- q^T, k^T (lane = token, registers = 4 head features), one after the other (register budget) ----
                // (head dim 16: the upper half of the 32-deep contraction is zero on both operands)
    #pragma unroll
                for (int which = 0; which < 2; ++which) {
                    const int nrt = Q1 && which == 0 ? 1 : NT;             // (constant once `which` is unrolled)
                    request_w(cur ^ 1, (which + 1) * E + h * DH);          // the next block: k after q, v after k
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 pa[DT][NT];
    #pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
    #pragma unroll
                        for (int dt = 0; dt < DT; ++dt)
    #pragma unroll
                            for (int rt = 0; rt < NT; ++rt)
                                if (rt < nrt) pa[dt][rt] = mma(wb[cur][ks][dt], xf[rt][ks], ks == 0 ? zero : pa[dt][rt]);
                    cur ^= 1;
    #pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        const f32x4 bb = ld4(bqkv + which * E + h * DH + 16 * dt + 4 * g);
    #pragma unroll
                        for (int rt = 0; rt < NT; ++rt)
                            if (rt < nrt) pa[dt][rt] += bb;
                    }
    #pragma unroll
                    for (int rt = 0; rt < NT; ++rt) {
                        if (rt >= nrt) continue;
                        if (which == 0) qf[rt] = pack8(pa[0][rt], DT == 2 ? pa[DT - 1][rt] : zero);
                        else kf[rt] = pack8(pa[0][rt], DT == 2 ? pa[DT - 1][rt] : zero);
                        if (EXTRAS) {          // (q leaves unscaled, as the reference's q_proj output)
                            const int off = vo_q[rt] + (which * E + h * DH) * 2;
                            if (which == 0) {
                                bst4_bf16(rqkv, off, pa[0][rt] * (1.f / QSCALE));
                                if (DT == 2) bst4_bf16(rqkv, off + 32, pa[DT - 1][rt] * (1.f / QSCALE));
                            } else if (DT == 2) bst_halves(rqkv, off, kf[rt]);          // k: exactly the packed operand
                            else bst_lo(rqkv, off, kf[rt]);
                        }
                    }
                }
                // ---- v (lane = head feature, registers = 4 tokens): the operand of P V with keys as contraction index ----
                {
                    if (h + 1 < H) request_w(cur ^ 1, (h + 1) * DH);          // q of the next head
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 va[NT][DT];
    #pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
    #pragma unroll
                        for (int dt = 0; dt < DT; ++dt)
    #pragma unroll
                            for (int rt = 0; rt < NT; ++rt) va[rt][dt] = mma(xf[rt][ks], wb[cur][ks][dt], ks == 0 ? zero : va[rt][dt]);
    #pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        const float bv = bqkv[2 * E + h * DH + 16 * dt + cq];
    #pragma unroll
                        for (int rt = 0; rt < NT; ++rt) va[rt][dt] += f32x4{bv, bv, bv, bv};
                    }
    #pragma unroll
                    for (int p = 0; p < NP; ++p)
    #pragma unroll
                        for (int dt = 0; dt < DT; ++dt) vr[p][dt] = pack8(va[2 * p][dt], (2 * p + 1 < NT) ? va[2 * p + 1][dt] : zero);
                    if (EXTRAS) {         // v^T once more (lane = token): 8-byte row stores instead of 2-byte scatters
    #pragma unroll
                        for (int dt = 0; dt < DT; ++dt) {
                            f32x4 vt[NT];
    #pragma unroll
                            for (int ks = 0; ks < KS; ++ks)
    #pragma unroll
                                for (int rt = 0; rt < NT; ++rt) vt[rt] = mma(wb[cur][ks][dt], xf[rt][ks], ks == 0 ? zero : vt[rt]);
                            const f32x4 bb = ld4(bqkv + 2 * E + h * DH + 16 * dt + 4 * g);
    #pragma unroll
                            for (int rt = 0; rt < NT; ++rt)
                                bst4_bf16(rqkv, vo_q[rt] + (2 * E + h * DH + 16 * dt) * 2, vt[rt] + bb);
                        }
                    }
                    cur ^= 1;
                }
            } else {
                __builtin_amdgcn_sched_barrier(0);
                // ---- q^T, k^T (lane = token, registers = 4 head features), one after the other (register budget) ----
                // (head dim 16: the upper half of the 32-deep contraction is zero on both operands)
    #pragma unroll
                for (int which = 0; which < 2; ++which) {
                    const int nrt = Q1 && which == 0 ? 1 : NT;             // (constant once `which` is unrolled)
                    f32x4 pa[DT][NT];
    #pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        const f32x4 bb = ld4(bqkv + which * E + h * DH + 16 * dt + 4 * g);
    #pragma unroll
                        for (int rt = 0; rt < NT; ++rt)
                            if (rt < nrt) pa[dt][rt] = bb;
                    }
    #pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
    #pragma unroll
                        for (int dt = 0; dt < DT; ++dt) {
                            const bf16x8 w = lds_frag(Wq + (which * E + h * DH + 16 * dt + cq) * LDE + ks * 32 + 8 * g);
    #pragma unroll
                            for (int rt = 0; rt < NT; ++rt)
                                if (rt < nrt) pa[dt][rt] = mma(w, xf[rt][ks], pa[dt][rt]);
                        }
    #pragma unroll
                    for (int rt = 0; rt < NT; ++rt) {
                        if (rt >= nrt) continue;
                        if (which == 0) qf[rt] = pack8(pa[0][rt], DT == 2 ? pa[DT - 1][rt] : zero);
                        else kf[rt] = pack8(pa[0][rt], DT == 2 ? pa[DT - 1][rt] : zero);
                        if (EXTRAS) {          // (q leaves unscaled, as the reference's q_proj output)
                            const int off = vo_q[rt] + (which * E + h * DH) * 2;
                            if (which == 0) {
                                bst4_bf16(rqkv, off, pa[0][rt] * (1.f / QSCALE));
                                if (DT == 2) bst4_bf16(rqkv, off + 32, pa[DT - 1][rt] * (1.f / QSCALE));
                            } else if (DT == 2) bst_halves(rqkv, off, kf[rt]);          // k: exactly the packed operand
                            else bst_lo(rqkv, off, kf[rt]);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                // ---- v (lane = head feature, registers = 4 tokens): the operand of P V with keys as contraction index ----
                {
                    f32x4 va[NT][DT];
    #pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        const float bv = bqkv[2 * E + h * DH + 16 * dt + cq];
    #pragma unroll
                        for (int rt = 0; rt < NT; ++rt) va[rt][dt] = f32x4{bv, bv, bv, bv};
                    }
    #pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
    #pragma unroll
                        for (int dt = 0; dt < DT; ++dt) {
                            const bf16x8 wv = lds_frag(Wq + (2 * E + h * DH + 16 * dt + cq) * LDE + ks * 32 + 8 * g);
    #pragma unroll
                            for (int rt = 0; rt < NT; ++rt) va[rt][dt] = mma(xf[rt][ks], wv, va[rt][dt]);
                        }
    #pragma unroll
                    for (int p = 0; p < NP; ++p)
    #pragma unroll
                        for (int dt = 0; dt < DT; ++dt) vr[p][dt] = pack8(va[2 * p][dt], (2 * p + 1 < NT) ? va[2 * p + 1][dt] : zero);
                    if (EXTRAS) {         // v^T once more (lane = token): 8-byte row stores instead of 2-byte scatters
    #pragma unroll
                        for (int dt = 0; dt < DT; ++dt) {
                            f32x4 vt[NT];
                            const f32x4 bb = ld4(bqkv + 2 * E + h * DH + 16 * dt + 4 * g);
    #pragma unroll
                            for (int rt = 0; rt < NT; ++rt) vt[rt] = bb;
    #pragma unroll
                            for (int ks = 0; ks < KS; ++ks) {
                                const bf16x8 wv = lds_frag(Wq + (2 * E + h * DH + 16 * dt + cq) * LDE + ks * 32 + 8 * g);
    #pragma unroll
                                for (int rt = 0; rt < NT; ++rt) vt[rt] = mma(wv, xf[rt][ks], vt[rt]);
                            }
    #pragma unroll
                            for (int rt = 0; rt < NT; ++rt)
                                bst4_bf16(rqkv, vo_q[rt] + (2 * E + h * DH + 16 * dt) * 2, vt[rt]);
                        }
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // ---- scores, softmax, P V per query tile ----
#pragma unroll
            for (int it = 0; it < NQ; ++it) {
                f32x4 st[NT];                        // S^T tile (log2 units): lane = query it*16 + cq, registers = keys 16 j + 4 g + r
                float m = -INFINITY;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    st[j] = mma(kf[j], qf[it], zero);
                    if (j == NT - 1) {               // only the last key tile can hold keys that do not exist
#pragma unroll
                        for (int r = 0; r < 4; ++r) st[j][r] = (j * 16 + 4 * g + r < S) ? st[j][r] : -INFINITY;
                    }
                    m = fmaxf(m, fmaxf(fmaxf(st[j][0], st[j][1]), fmaxf(st[j][2], st[j][3])));
                }
                m = x4_max(m);
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        st[j][r] = __builtin_amdgcn_exp2f(st[j][r] - m);      // exp2(-inf) = 0 for the masked keys
                        sum += st[j][r];
                    }
                const float inv = __builtin_amdgcn_rcpf(x4_sum(sum));
#pragma unroll
                for (int j = 0; j < NT; ++j) st[j] *= inv;
                f32x4 ot[DT];                        // O^T: lane = query, registers = head features 16 dt + 4 g + r
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) ot[dt] = zero;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const bf16x8 pf = pack8(st[2 * p], (2 * p + 1 < NT) ? st[2 * p + 1] : zero);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) ot[dt] = mma(vr[p][dt], pf, ot[dt]);
                }
                if (DT == 1 && (h & 1) == 0) { ot_even[it] = ot[0]; continue; }        // (stored with its odd neighbour)
                const int kb = h / HB;                                               // the 32-feature block this head completes
                cf[kb][it] = DT == 2 ? pack8(ot[0], ot[DT - 1]) : pack8(ot_even[it], ot[0]);
                bst_halves(rctx, vo_e[it] + kb * 64, cf[kb][it]);
            }
        }
        request(min(b + bstride, a.B - 1));      // (unconditional: a clamped re-read on the last round)
        __builtin_amdgcn_sched_barrier(0);
        // ---- out-projection (+ bias) + residual (identity product on the input fragments), LayerNorm ----
        f32x4 oa[ET][NT];
        if constexpr (WIDE) {
            // the same one-block-ahead batches for the out-projection's fragments (ET reads per 32-feature block); the residual's
            // bias / gamma vectors as one batch in front of the identity products they scale
            bf16x8 wo[2][ET];
            auto request_wo = [&](int buf, int kb) {
#pragma unroll
                for (int nt = 0; nt < ET; ++nt) wo[buf][nt] = lds_frag(Wo + (16 * nt + cq) * LDE + kb * 32 + 8 * g);
            };
            f32x4 bvs[ET], gvs[ET];
#pragma unroll
            for (int nt = 0; nt < ET; ++nt) { bvs[nt] = ld4(bo + 16 * nt + 4 * g); gvs[nt] = ld4(gin + 16 * nt + 4 * g); }
            request_wo(0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nt = 0; nt < ET; ++nt)
#pragma unroll
                for (int rt = 0; rt < NQ; ++rt) oa[nt][rt] = bvs[nt] + gvs[nt] * mma((nt & 1) ? id1 : id0, xf[rt][nt >> 1], zero);
#pragma unroll
            for (int kb = 0; kb < KS; ++kb) {
                if (kb + 1 < KS) request_wo((kb + 1) & 1, kb + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nt = 0; nt < ET; ++nt)
#pragma unroll
                    for (int rt = 0; rt < NQ; ++rt) oa[nt][rt] = mma(wo[kb & 1][nt], cf[kb][rt], oa[nt][rt]);
            }
        } else {
#pragma unroll
            for (int nt = 0; nt < ET; ++nt) {
                const f32x4 bv = ld4(bo + 16 * nt + 4 * g), gv = ld4(gin + 16 * nt + 4 * g);
#pragma unroll
                for (int rt = 0; rt < NQ; ++rt) oa[nt][rt] = bv + gv * mma((nt & 1) ? id1 : id0, xf[rt][nt >> 1], zero);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kb = 0; kb < KS; ++kb) {
#pragma unroll
                for (int nt = 0; nt < ET; ++nt) {
                    const bf16x8 w = lds_frag(Wo + (16 * nt + cq) * LDE + kb * 32 + 8 * g);
#pragma unroll
                    for (int rt = 0; rt < NQ; ++rt) oa[nt][rt] = mma(w, cf[kb][rt], oa[nt][rt]);
                }
                __builtin_amdgcn_sched_barrier(0);      // keeps the weight-fragment reads of later heads from piling up
            }
        }
#pragma unroll
        for (int rt = 0; rt < NQ; ++rt) {
            f32x4 z[ET];
#pragma unroll
            for (int nt = 0; nt < ET; ++nt) z[nt] = oa[nt][rt];
            ln_store(z, dst, vo_e[rt], vo_r[rt], gout, bout);
        }
        if constexpr (Q1) {
            if (has_qkv) {          // the backward's feed-forward block reads every row of the normalised output: zeros behind tile 0
#pragma unroll
                for (int rt = 1; rt < NT; ++rt)
#pragma unroll
                    for (int i = 0; i < KS; ++i) __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{0u, 0u, 0u, 0u}, dst.n, vo_l[rt] + 64 * i, 0, 0);
            }
        }
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename Kern>
int set_lds(Kern k, int bytes) {
    MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return 0;
}

}  // namespace

bool fused_layer_supported(int dtype, int E_, int F_, int H_, int S) {
    static const bool off = getenv("MIVIT_NO_FUSED_LAYER") != nullptr;
    return !off && dtype == MIVIT_ELEM_DTYPE && E_ == E && F_ == F && H_ == H && S >= 1 && S <= 64;
}

int launch_mlp_block_fwd(const void *nin, const float *gin, const float *bin, const void *W1, const float *b1, const void *W2,
                         const float *b2, const float *gout, const float *bout, int M, int act, void *nout, float *rstd,
                         void *xout, void *zout, float *mean, void *hout, void *uout, hipStream_t s) {
    MIVIT_CHECK(nin && W1 && b1 && W2 && b2 && nout && rstd && M > 0, "mlp_block_fwd: null pointer / empty problem");
    MIVIT_CHECK((gin == nullptr) == (bin == nullptr), "mlp_block_fwd: input affine needs both gamma and beta");
    MIVIT_CHECK(!xout || (gout && bout), "mlp_block_fwd: xout needs the LayerNorm affine");
    MIVIT_CHECK(aligned16(nin) && aligned16(W1) && aligned16(W2) && aligned16(nout) && aligned16(xout) && aligned16(zout) &&
                aligned16(hout) && aligned16(uout), "mlp_block_fwd: pointers must be 16-byte aligned");
    MlpFwdArgs a{};
    a.nin = static_cast<const bf16 *>(nin); a.gin = gin; a.bin = bin;
    a.W1 = static_cast<const bf16 *>(W1); a.b1 = b1; a.W2 = static_cast<const bf16 *>(W2); a.b2 = b2;
    a.gout = gout; a.bout = bout; a.M = M; a.act = act;
    a.o = LnOut{static_cast<bf16 *>(nout), rstd, static_cast<bf16 *>(xout), static_cast<bf16 *>(zout), mean};
    a.hout = static_cast<bf16 *>(hout); a.uout = static_cast<bf16 *>(uout);
    // 32 rows per wave, 8 waves per workgroup (two per SIMD, 230 registers).  Round 3 measured the other end of the trade: 16 rows
    // per wave with 12 waves (161 registers, three per SIMD; every weight fragment then feeds one MFMA instead of two, twice the
    // LDS reads per row): 99.4 against 101.5 us per layer -- no difference; with 16 waves (128 registers) it spills 31: 126.7 us.
    constexpr int NR = 2;
    const int ntiles = ceil_div(M, 16 * NR);
    const int grid = std::min(256, ceil_div(ntiles, NWAVES));
    const bool extras = hout || uout;
    ProfScope prof(s);
#define MLP_LAUNCH(ACT_, EX_)                                                                    \
    do {                                                                                         \
        auto kern = mlp_block_fwd_kernel<NR, ACT_, EX_>;                                         \
        RC(set_lds(kern, MLP_LDS));                                                              \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NTHREADS), MLP_LDS, s, a);                     \
    } while (0)
#define MLP_ACT(ACT_) do { if (extras) MLP_LAUNCH(ACT_, true); else MLP_LAUNCH(ACT_, false); } while (0)
    switch (act) {
        case MIVIT_ACT_RELU: MLP_ACT(MIVIT_ACT_RELU); break;
        case MIVIT_ACT_LEAKY_RELU: MLP_ACT(MIVIT_ACT_LEAKY_RELU); break;
        case MIVIT_ACT_GELU: MLP_ACT(MIVIT_ACT_GELU); break;
        default: MLP_ACT(MIVIT_ACT_NONE); break;
    }
#undef MLP_ACT
#undef MLP_LAUNCH
    MIVIT_LAUNCH_CHECK();
    return 0;
}

int launch_attn_block_fwd(const void *nin, const float *gin, const float *bin, const void *Wqkv, const float *bqkv,
                          const void *Wo, const float *bo, const float *gout, const float *bout, int B, int S, void *ctx,
                          void *nout, float *rstd, void *xout, void *zout, float *mean, void *qkvout, bool q1, hipStream_t s) {
    MIVIT_CHECK(nin && Wqkv && bqkv && Wo && bo && ctx && nout && rstd && B > 0, "attn_block_fwd: null pointer / empty problem");
    MIVIT_CHECK(S >= 1 && S <= 64, "attn_block_fwd: %d tokens per sequence (supported: 1..64)", S);
    MIVIT_CHECK((gin == nullptr) == (bin == nullptr), "attn_block_fwd: input affine needs both gamma and beta");
    MIVIT_CHECK(!xout || (gout && bout), "attn_block_fwd: xout needs the LayerNorm affine");
    MIVIT_CHECK(aligned16(nin) && aligned16(Wqkv) && aligned16(Wo) && aligned16(ctx) && aligned16(nout) && aligned16(xout) &&
                aligned16(zout) && aligned16(qkvout), "attn_block_fwd: pointers must be 16-byte aligned");
    AttnFwdArgs a{};
    a.nin = static_cast<const bf16 *>(nin); a.gin = gin; a.bin = bin;
    a.Wqkv = static_cast<const bf16 *>(Wqkv); a.bqkv = bqkv; a.Wo = static_cast<const bf16 *>(Wo); a.bo = bo;
    a.gout = gout; a.bout = bout; a.B = B; a.S = S; a.ctx = static_cast<bf16 *>(ctx);
    a.o = LnOut{static_cast<bf16 *>(nout), rstd, static_cast<bf16 *>(xout), static_cast<bf16 *>(zout), mean};
    a.qkvout = static_cast<bf16 *>(qkvout);
    const int nt = ceil_div(S, 16);
    static const int nw_env = [] { const char *e = getenv("MIVIT_ATTN_BLOCK_WAVES"); return e ? atoi(e) : 0; }();
    // waves per workgroup (measured, scripts/bench_fused.py): width 128 -- four (one per SIMD, 242-386 registers) for three and four
    // row tiles and for every training launch (with the q|k|v store, 31 tokens: 245 against 284 us; 16 tokens: 132 against 163),
    // eight for the lean forward of one or two tiles (151 against 169 us); width 64 -- eight throughout
    // (the one-query-tile variant was measured at both counts too: three tiles with the q|k|v store, four waves 8.156 / 8.122 ms per
    //  step against eight 8.187 / 8.135 -- the same rule)
    const int nw = nw_env == 8 || nw_env == 4 ? nw_env : (E == 128 && (nt >= 3 || qkvout) ? 4 : 8);
    const int grid = std::min(256, ceil_div(B, nw));
    ProfScope prof(s);
    // q1: the query side for row tile 0 only (attn_block_fwd_kernel, Q1); one row tile: that is the whole sequence
#define ATT_LAUNCH3(NT_, EX_, NW_)                                                               \
    do {                                                                                         \
        auto kern = q1 && NT_ > 1 ? attn_block_fwd_kernel<NT_, EX_, NW_, (NT_ > 1)> : attn_block_fwd_kernel<NT_, EX_, NW_, false>; \
        RC(set_lds(kern, ATT_LDS));                                                              \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NW_ * 64), ATT_LDS, s, a);                     \
    } while (0)
#define ATT_LAUNCH(NT_)                                                                          \
    do {                                                                                         \
        if (qkvout) { if (nw == 8) ATT_LAUNCH3(NT_, true, 8); else ATT_LAUNCH3(NT_, true, 4); }  \
        else { if (nw == 8) ATT_LAUNCH3(NT_, false, 8); else ATT_LAUNCH3(NT_, false, 4); }       \
    } while (0)
    switch (nt) {
        case 1: ATT_LAUNCH(1); break;
        case 2: ATT_LAUNCH(2); break;
        case 3: ATT_LAUNCH(3); break;
        default: ATT_LAUNCH(4); break;
    }
#undef ATT_LAUNCH
#undef ATT_LAUNCH3
    MIVIT_LAUNCH_CHECK();
    return 0;
}

// ---- operator-level C-ABI (tests, external callers; include/mivit_hip.h): one set per build, named by elem.h ----
extern "C" int mivit_fused_layer_supported(int dtype, int embed_dim, int hidden_dim, int num_heads, int tokens) {
    return fused_layer_supported(dtype, embed_dim, hidden_dim, num_heads, tokens) ? 1 : 0;
}
extern "C" int mivit_mlp_block_fwd(const void *n_in, const float *gamma_in, const float *beta_in, const void *W1_bf16,
                                   const float *b1, const void *W2_bf16, const float *b2, const float *gamma_out,
                                   const float *beta_out, int M, int act, void *n_out, float *rstd, void *x_out, void *z_out,
                                   float *mean, void *h_out, void *u_out, void *stream) {
    prof_set_tag(MIVIT_PROF_OP);
    return launch_mlp_block_fwd(n_in, gamma_in, beta_in, W1_bf16, b1, W2_bf16, b2, gamma_out, beta_out, M, act, n_out, rstd,
                                x_out, z_out, mean, h_out, u_out, static_cast<hipStream_t>(stream));
}
extern "C" int mivit_attn_block_fwd(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv_bf16,
                                    const float *bqkv, const void *Wo_bf16, const float *bo, const float *gamma_out,
                                    const float *beta_out, int B, int S, void *ctx, void *n_out, float *rstd, void *x_out,
                                    void *z_out, float *mean, void *qkv_out, void *stream) {
    prof_set_tag(MIVIT_PROF_OP);
    return launch_attn_block_fwd(n_in, gamma_in, beta_in, Wqkv_bf16, bqkv, Wo_bf16, bo, gamma_out, beta_out, B, S, ctx, n_out,
                                 rstd, x_out, z_out, mean, qkv_out, false, static_cast<hipStream_t>(stream));
}
extern "C" int mivit_attn_block_fwd_q1(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv_bf16,
                                       const float *bqkv, const void *Wo_bf16, const float *bo, const float *gamma_out,
                                       const float *beta_out, int B, int S, void *ctx, void *n_out, float *rstd, void *x_out,
                                       void *z_out, float *mean, void *qkv_out, void *stream) {
    prof_set_tag(MIVIT_PROF_OP);
    return launch_attn_block_fwd(n_in, gamma_in, beta_in, Wqkv_bf16, bqkv, Wo_bf16, bo, gamma_out, beta_out, B, S, ctx, n_out,
                                 rstd, x_out, z_out, mean, qkv_out, true, static_cast<hipStream_t>(stream));
}
