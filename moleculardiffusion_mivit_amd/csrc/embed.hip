// HBM-streaming kernels of the frame embedding (bf16 mode): the two launches that read the fp32 frames.
//
//   forward : emb[M, E]  = X[M, K] . W[E, K]^T + b          X = fp32 frames [B*T, P*P], W = bf16 shadow weights
//   wgrad   : dW[E, K]   = sum_m d_emb[m, :]^T X[m, :]      (split over rows into fp32 slabs, reduced deterministically)
//
// Both are bound by the one pass over X (AI = E/2 FLOP/B), so the design goal is bytes in flight, not FLOPs:
//  * operands go global -> LDS by LDS-DMA (global_load_lds, 16 B per lane, 1 KiB per wave-instruction): no staging
//    registers, a 3-slot ring with two stages in flight behind counted s_waitcnt vmcnt + raw s_barrier;
//  * fp32 -> bf16 conversion happens AFTER the LDS read, on the MFMA operand fragments;
//  * LDS images are the natural row-major tiles; bank conflicts are removed by XOR-permuting the 16-byte chunks of
//    a row on the SOURCE address (the DMA destination is lane-linear) and applying the same XOR when reading;
//  * in wgrad the contraction runs over rows: the bf16 operand is read with ds_read_b64_tr_b16, the fp32 operand
//    with 8 scalar reads per fragment (no 32-bit transposing read exists).
// Shapes outside the constraints below fall back to the general register-staged GEMM (gemm.hip).
#include "common.h"
#include "stream_prims.h"
#include <stdlib.h>
#include "elem.h"          // element type of this translation unit (bf16, or f16 under -DMIVIT_ELEM_F16): after every other include

namespace {



__device__ __forceinline__ bf16x8 cvt8(const float4 a, const float4 b) {
    bf16x8 f;
    f[0] = (__bf16)a.x; f[1] = (__bf16)a.y; f[2] = (__bf16)a.z; f[3] = (__bf16)a.w;
    f[4] = (__bf16)b.x; f[5] = (__bf16)b.y; f[6] = (__bf16)b.z; f[7] = (__bf16)b.w;
    return f;
}

constexpr int NSLOT = 3;

// =================================================================================================================
// forward: tile BM rows x 128 columns, stage = 64 fp32 k of X (256 B rows) + 64 bf16 k of W (128 B rows).
// BM / 64 x 2 waves, each owning a 64 x 64 sub-tile.  NS ring slots, NS - 1 stages in flight.
// =================================================================================================================
template <int BM, int NS>
struct FwdCfg {
    static constexpr int BN = 128, BK = 64;
    static constexpr int NW = BM / 64 * 2;               // waves per block
    static constexpr int A_BYTES = BM * BK * 4;
    static constexpr int B_BYTES = BN * BK * 2;          // 16 KiB
    static constexpr int STAGE = A_BYTES + B_BYTES;
    static constexpr int A_DMA = A_BYTES / 1024 / NW;    // wave-instructions per wave per stage
    static constexpr int B_DMA = B_BYTES / 1024 / NW;
    static constexpr int PER_STAGE = A_DMA + B_DMA;
    static_assert(A_DMA * NW * 1024 == A_BYTES && B_DMA * NW * 1024 == B_BYTES, "stage must split evenly over the waves");
};

struct EmbFwdArgs {
    const float *X; const bf16 *W; const float *bias; bf16 *Y;
    int M, K, E;
    int kstag;      // direct kernel: workgroup y starts its k loop at stage (y * kstag) % stages (spreads the HBM channels)
};

template <int BM, int NS>
__device__ __forceinline__ void fwd_issue(const EmbFwdArgs &a, unsigned char *slot, int m0, int n0, int k0, int wave,
                                          int lane) {
    using C = FwdCfg<BM, NS>;
    // A: 4 rows (256 B each) per wave-instruction; chunk c of row r lands in slot c ^ (2 * (r & 7))
#pragma unroll
    for (int i = 0; i < C::A_DMA; ++i) {
        const int inst = wave * C::A_DMA + i;
        const int r = inst * 4 + (lane >> 4), s = lane & 15;
        const int c = s ^ (2 * (r & 7));
        const int gr = min(m0 + r, a.M - 1);
        dma16(a.X + (int64_t)gr * a.K + k0 + c * 4, slot + inst * 1024);
    }
    // B: 8 rows (128 B each) per wave-instruction; chunk c of row n lands in slot c ^ ((n >> 1) & 7)
    unsigned char *bs = slot + C::A_BYTES;
#pragma unroll
    for (int i = 0; i < C::B_DMA; ++i) {
        const int inst = wave * C::B_DMA + i;
        const int n = inst * 8 + (lane >> 3), s = lane & 7;
        const int c = s ^ ((n >> 1) & 7);
        dma16(a.W + (int64_t)(n0 + n) * a.K + k0 + c * 8, bs + inst * 1024);
    }
}

template <int BM, int NS>
__global__ __launch_bounds__(BM / 64 * 2 * 64) void embed_fwd_dma(const EmbFwdArgs a) {
    using C = FwdCfg<BM, NS>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TM = 4, TN = 4, BN = C::BN, NT = C::NW * 64;
    constexpr int D = NS - 1;                      // prefetch distance (stages in flight)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int nst = a.K / C::BK;
    const int g = lane >> 4, cq = lane & 15;

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s = 0; s < D; ++s)
        if (s < nst) fwd_issue<BM, NS>(a, smem + s * C::STAGE, m0, n0, s * C::BK, wave, lane);
    for (int s = 0; s < nst; ++s) {
        // stage s has landed once only the younger in-flight stages of this wave's DMAs remain outstanding
        if (s + D - 1 < nst) wait_vm<C::PER_STAGE * (D - 1)>();
        else wait_vm<0>();
        barrier();      // everyone's share of stage s landed; everyone finished reading the slot of stage s-1
        if (s + D < nst) fwd_issue<BM, NS>(a, smem + ((s + D) % NS) * C::STAGE, m0, n0, (s + D) * C::BK, wave, lane);
        const unsigned char *As = smem + (s % NS) * C::STAGE, *Bs = As + C::A_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int r = wm * 64 + i * 16 + cq;
                const int c = (kk * 8 + 2 * g) ^ (2 * (r & 7));
                const float4 *p = reinterpret_cast<const float4 *>(As + r * 256 + c * 16);
                af[i] = cvt8(p[0], p[1]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = wn * 64 + j * 16 + cq;
                const int c = (kk * 4 + g) ^ ((n >> 1) & 7);
                bf[j] = *reinterpret_cast<const bf16x8 *>(Bs + n * 128 + c * 16);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mma(af[i], bf[j], acc[i][j]);
        }
    }
    // epilogue: + bias, through LDS as fp32 (64 rows per pass = the rows of one wave row), 16-byte bf16 stores
    constexpr int LDC = BN + 4;
    float *Cs = reinterpret_cast<float *>(smem);
    for (int h = 0; h < BM / 64; ++h) {
        barrier();
        if (wm == h) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int lc = wn * 64 + j * 16 + cq;
                    const float bv = a.bias ? a.bias[n0 + lc] : 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) Cs[(i * 16 + 4 * g + r) * LDC + lc] = acc[i][j][r] + bv;
                }
        }
        barrier();
        for (int c = tid; c < 64 * (BN / 8); c += NT) {
            const int lr = c / (BN / 8), lc = (c % (BN / 8)) * 8;
            const int row = m0 + h * 64 + lr;
            if (row < a.M) {
                float v[8];
                *reinterpret_cast<float4 *>(v) = *reinterpret_cast<const float4 *>(Cs + lr * LDC + lc);
                *reinterpret_cast<float4 *>(v + 4) = *reinterpret_cast<const float4 *>(Cs + lr * LDC + lc + 4);
                store16(a.Y + (int64_t)row * a.E + n0 + lc, v);
            }
        }
    }
}

// =================================================================================================================
// forward, LDS-DMA with 32-k stages: 256 rows x 128 columns per workgroup (8 waves, 64 x 64 each), stage = 32 fp32 k of X
// (128-byte rows) + 32 bf16 k of W (64-byte rows) = 40 KB, two slots = 80 KB -> TWO workgroups (16 waves) per CU.
// =================================================================================================================
struct F32Cfg {
    static constexpr int BM = 256, BN = 128, BK = 32, NW = 8, NS = 2;
    static constexpr int A_BYTES = BM * BK * 4, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    static constexpr int A_DMA = A_BYTES / 1024 / NW, B_DMA = B_BYTES / 1024 / NW;     // 4, 1
};

__device__ __forceinline__ void f32_issue(const EmbFwdArgs &a, unsigned char *slot, int m0, int n0, int k0, int wave, int lane) {
    using C = F32Cfg;
    // A: 8 rows (128 B) per wave-instruction; the 32-byte chunk PAIR p of row r lands in pair slot p ^ ((r >> 1) & 3)
#pragma unroll
    for (int i = 0; i < C::A_DMA; ++i) {
        const int inst = wave * C::A_DMA + i;
        const int r = inst * 8 + (lane >> 3), sl = lane & 7;
        const int c = (((sl >> 1) ^ ((r >> 1) & 3)) << 1) | (sl & 1);
        dma16(a.X + (int64_t)min(m0 + r, a.M - 1) * a.K + k0 + c * 4, slot + inst * 1024);
    }
    // B: 16 rows (64 B) per wave-instruction; chunk c of row n lands in slot c ^ ((n >> 2) & 3)
    unsigned char *bs = slot + C::A_BYTES;
    {
        const int n = wave * 16 + (lane >> 2), sl = lane & 3;
        const int c = sl ^ ((n >> 2) & 3);
        dma16(a.W + (int64_t)(n0 + n) * a.K + k0 + c * 8, bs + wave * 1024);
    }
}

__global__ __launch_bounds__(512, 4) void embed_fwd_dma32(const EmbFwdArgs a) {
    using C = F32Cfg;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TM = 4, TN = 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * C::BM, n0 = blockIdx.x * C::BN;
    const int nst = a.K / C::BK;
    const int g = lane >> 4, cq = lane & 15;
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32_issue(a, smem, m0, n0, 0, wave, lane);
    for (int s = 0; s < nst; ++s) {
        wait_vm<0>();
        barrier();      // stage s landed everywhere; everyone finished reading the other slot
        if (s + 1 < nst) f32_issue(a, smem + ((s + 1) & 1) * C::STAGE, m0, n0, (s + 1) * C::BK, wave, lane);
        const unsigned char *As = smem + (s & 1) * C::STAGE, *Bs = As + C::A_BYTES;
        bf16x8 af[TM], bf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int r = wm * 64 + i * 16 + cq;
            const float4 *p = reinterpret_cast<const float4 *>(As + r * 128 + ((g ^ ((r >> 1) & 3)) << 5));
            af[i] = cvt8(p[0], p[1]);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = wn * 64 + j * 16 + cq;
            bf[j] = *reinterpret_cast<const bf16x8 *>(Bs + n * 64 + ((g ^ ((n >> 2) & 3)) << 4));
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = mma(af[i], bf[j], acc[i][j]);
    }
    // epilogue: + bias, through LDS as fp32 (64 rows per pass), 16-byte bf16 stores
    constexpr int LDC = C::BN + 4;
    float *Cs = reinterpret_cast<float *>(smem);
    for (int h = 0; h < C::BM / 64; ++h) {
        barrier();
        if (wm == h) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int lc = wn * 64 + j * 16 + cq;
                    const float bv = a.bias ? a.bias[n0 + lc] : 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) Cs[(i * 16 + 4 * g + r) * LDC + lc] = acc[i][j][r] + bv;
                }
        }
        barrier();
        for (int c = tid; c < 64 * (C::BN / 8); c += 512) {
            const int lr = c / (C::BN / 8), lc = (c % (C::BN / 8)) * 8;
            const int row = m0 + h * 64 + lr;
            if (row < a.M) {
                float v[8];
                *reinterpret_cast<float4 *>(v) = *reinterpret_cast<const float4 *>(Cs + lr * LDC + lc);
                *reinterpret_cast<float4 *>(v + 4) = *reinterpret_cast<const float4 *>(Cs + lr * LDC + lc + 4);
                store16(a.Y + (int64_t)row * a.E + n0 + lc, v);
            }
        }
    }
}

// =================================================================================================================
// forward, "direct" variant: the fp32 frames never touch LDS.  Each wave owns 32 rows x 128 columns and loads its X
// fragments straight from global memory into the MFMA operand registers, one 64-k stage ahead (8 x 16-byte loads per
// lane in flight, no barrier on that path, 12 waves per CU -> ~100 KB of X in flight per CU).  Only the bf16 W tile
// [128][64] goes through a 3-slot LDS ring by DMA.  The k order inside a 32-k MFMA step is permuted so that the four
// lane groups of a row read one contiguous 64-byte run per load instruction:
//      lane group g holds k = 4g..4g+3 and 16+4g..16+4g+3   (X: two float4 loads; W: two 8-byte LDS reads)
// =================================================================================================================
// TMW = 16-row tiles per wave (accumulators 32 * TMW registers), NW waves per workgroup, NS ring slots of the W tile
template <int TMW, int NW_, int NS_>
struct DirCfg {
    static constexpr int NW = NW_, NS = NS_, BM = NW * 16 * TMW, BN = 128, BK = 64;
    static constexpr int B_BYTES = BN * BK * 2;                  // 16 KiB per stage
    static constexpr int B_DMA = B_BYTES / 1024 / NW;            // wave-instructions per wave per stage
    static constexpr int A_LD = 4 * TMW;                         // global loads per wave per stage (TMW tiles x 2 kk x 2)
    static_assert(B_DMA * NW * 1024 == B_BYTES, "W stage must split evenly over the waves");
};

template <int NW>
__device__ __forceinline__ void dir_issue_b(const EmbFwdArgs &a, unsigned char *slot, int n0, int k0, int wave, int lane) {
    constexpr int B_DMA = 128 * 64 * 2 / 1024 / NW;
#pragma unroll
    for (int i = 0; i < B_DMA; ++i) {
        const int inst = wave * B_DMA + i;
        const int n = inst * 8 + (lane >> 3), sl = lane & 7;
        const int c = sl ^ ((n >> 1) & 7);
        dma16(a.W + (int64_t)(n0 + n) * a.K + k0 + c * 8, slot + inst * 1024);
    }
}

template <int TMW, int NW, int NS>
__global__ __launch_bounds__(NW * 64) void embed_fwd_direct(const EmbFwdArgs a) {
    using C = DirCfg<TMW, NW, NS>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int D = NS - 1;                                     // W stages in flight
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, cq = lane & 15;
    const int m0 = blockIdx.y * C::BM, n0 = blockIdx.x * C::BN, nst = a.K / C::BK;
    // Rows are K * 4 bytes apart (16 KB at P = 64), a multiple of the HBM channel interleave: workgroups that walk k in step
    // all sit on the same few channels.  Each workgroup therefore starts at its own stage and wraps (the sum over k is the
    // same set of products; only the fp32 accumulation order differs, deterministically per workgroup).
    const int s0 = (int)(((unsigned)blockIdx.y * (unsigned)a.kstag) % (unsigned)nst);
    auto stage_k = [&](int s) { int t = s + s0; t = t >= nst ? t - nst : t; return t * C::BK; };
    const float *ap[TMW];
#pragma unroll
    for (int i = 0; i < TMW; ++i) ap[i] = a.X + (int64_t)min(m0 + (wave * TMW + i) * 16 + cq, a.M - 1) * a.K + 4 * g;

    f32x4 acc[TMW][8];
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float4 nx[2][TMW][2];                                        // [kk][tile][half]: the next stage's frame fragments
    auto load_a = [&](int k0, float4 (&dst)[2][TMW][2]) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < TMW; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h) dst[kk][i][h] = *reinterpret_cast<const float4 *>(ap[i] + k0 + 32 * kk + 16 * h);
    };
#pragma unroll
    for (int s = 0; s < D; ++s)
        if (s < nst) dir_issue_b<NW>(a, smem + s * C::B_BYTES, n0, stage_k(s), wave, lane);
    load_a(stage_k(0), nx);
    for (int s = 0; s < nst; ++s) {
        float4 cx[2][TMW][2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < TMW; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h) cx[kk][i][h] = nx[kk][i][h];
        // The frame loads are ordinary loads: the compiler orders their uses itself.  The explicit wait is for W stage s (the
        // LDS-DMA is invisible to the compiler).  VM program order of a wave (A = A_LD frame loads, W = B_DMA DMA pieces):
        //   prologue W(0) .. W(D-1) A(0);   iteration i:  A(i+1) | wait | barrier | W(i+D) if it exists | compute(i)
        // W(s) was issued in iteration s - D (or the prologue); younger than it are A(s-D+2) .. A(s+1) -- at least A(s+1) --
        // and W(s+1) .. W(s+D-1) where those exist.  The count used is the minimum over all s: the youngest frame stage plus,
        // when W(s+D-1) was issued, the D - 1 younger W stages.
        load_a(stage_k(min(s + 1, nst - 1)), nx);
        if (s + D - 1 < nst) wait_vm<C::A_LD + (D - 1) * C::B_DMA>();
        else wait_vm<C::A_LD>();
        barrier();          // every wave's share of W stage s landed; every wave finished reading the slot of stage s-1
        if (s + D < nst) dir_issue_b<NW>(a, smem + ((s + D) % NS) * C::B_BYTES, n0, stage_k(s + D), wave, lane);
        const unsigned char *Bs = smem + (s % NS) * C::B_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[TMW];
#pragma unroll
            for (int i = 0; i < TMW; ++i) af[i] = cvt8(cx[kk][i][0], cx[kk][i][1]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int n = j * 16 + cq, sw = (n >> 1) & 7;
                const unsigned char *row = Bs + n * 128 + 8 * (g & 1);
                // volatile: keeps these as ds_read_b64 (64-bank rule, this image is conflict-free under it).  Left alone the
                // compiler pairs the reads of two column tiles into ds_read2st64_b64, which banks modulo 32 and runs at half the
                // rate: lanes cq and cq ^ 1 (rows 128 B apart) then collide -- SQ_LDS_BANK_CONFLICT 0.49 of the LDS-active cycles
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                typedef __attribute__((address_space(3))) const volatile u32x2 lds_u32x2;
                const u32x2 lo = *(lds_u32x2 *)(row + ((4 * kk + (g >> 1)) ^ sw) * 16);
                const u32x2 hi = *(lds_u32x2 *)(row + ((4 * kk + 2 + (g >> 1)) ^ sw) * 16);
                const bf16x8 bf = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
#pragma unroll
                for (int i = 0; i < TMW; ++i) acc[i][j] = mma(af[i], bf, acc[i][j]);
            }
        }
    }
    // epilogue: + bias, through LDS as fp32, one 16-row tile per wave per pass, 16-byte bf16 stores
    constexpr int LDC = C::BN + 4;
    float *Cs = reinterpret_cast<float *>(smem) + wave * 16 * LDC;
    float bv[8];                   // (one batch of loads: see embed_fwd_direct2)
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = 0.f;
    if (a.bias) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = a.bias[n0 + j * 16 + cq];
    }
#pragma unroll
    for (int i = 0; i < TMW; ++i) {
        barrier();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int lc = j * 16 + cq;
#pragma unroll
            for (int r = 0; r < 4; ++r) Cs[(4 * g + r) * LDC + lc] = acc[i][j][r] + bv[j];
        }
        barrier();
        for (int c = lane; c < 16 * (C::BN / 8); c += 64) {
            const int lr = c / (C::BN / 8), lc = (c % (C::BN / 8)) * 8;
            const int row = m0 + (wave * TMW + i) * 16 + lr;
            if (row < a.M) {
                float v[8];
                *reinterpret_cast<float4 *>(v) = *reinterpret_cast<const float4 *>(Cs + lr * LDC + lc);
                *reinterpret_cast<float4 *>(v + 4) = *reinterpret_cast<const float4 *>(Cs + lr * LDC + lc + 4);
                store16(a.Y + (int64_t)row * a.E + n0 + lc, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same kernel with the frame loads written out (inline asm) and two register stages swapped by a 2x unrolled loop.
// With ordinary loads the compiler places its own wait for the previous stage's registers, s_waitcnt vmcnt(8): it counts
// the 8 loads of the next stage issued since -- but not the 4 W-tile DMA pieces issued after them (they are inline asm too,
// stream_prims.h::dma16), so that wait also drains the four OLDEST loads of the stage it has just requested: half of the
// one-stage-ahead prefetch was being waited for every stage.  Here nothing in the loop is visible to the compiler's
// waitcnt pass; the order is the explicit  load A(s+1) -> wait_vm<A_LD + (D-1) * B_DMA>() -> barrier  of the kernel above,
// and there is no register copy between the stages (a copy would read registers whose loads are still in flight).
// ---------------------------------------------------------------------------------------------------------------------
template <int TMW, int NW, int NS>
__global__ __launch_bounds__(NW * 64) void embed_fwd_direct2(const EmbFwdArgs a) {
    using C = DirCfg<TMW, NW, NS>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int D = NS - 1;
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, cq = lane & 15;
    const int m0 = blockIdx.y * C::BM, n0 = blockIdx.x * C::BN, nst = a.K / C::BK;
    const int s0 = (int)(((unsigned)blockIdx.y * (unsigned)a.kstag) % (unsigned)nst);
    auto stage_k = [&](int s) { int t = s + s0; t = t >= nst ? t - nst : t; return t * C::BK; };
    const float *ap[TMW];
#pragma unroll
    for (int i = 0; i < TMW; ++i) ap[i] = a.X + (int64_t)min(m0 + (wave * TMW + i) * 16 + cq, a.M - 1) * a.K + 4 * g;

    f32x4 acc[TMW][8];
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto load_a = [&](int k0, f32x4_t (&dst)[2][TMW][2]) {      // one address pair per row tile, the four pieces by immediate offset
#pragma unroll
        for (int i = 0; i < TMW; ++i) {
            const float *base = ap[i] + k0;
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst[0][i][0]) : "v"(base) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, off offset:64" : "=v"(dst[0][i][1]) : "v"(base) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, off offset:128" : "=v"(dst[1][i][0]) : "v"(base) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, off offset:192" : "=v"(dst[1][i][1]) : "v"(base) : "memory");
        }
    };
    auto compute = [&](const unsigned char *Bs, f32x4_t (&cx)[2][TMW][2]) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[TMW];
#pragma unroll
            for (int i = 0; i < TMW; ++i) {
                asm volatile("" : "+v"(cx[kk][i][0]), "+v"(cx[kk][i][1]));          // (ordered after the wait above)
                const float4 lo = make_float4(cx[kk][i][0][0], cx[kk][i][0][1], cx[kk][i][0][2], cx[kk][i][0][3]);
                const float4 hi = make_float4(cx[kk][i][1][0], cx[kk][i][1][1], cx[kk][i][1][2], cx[kk][i][1][3]);
                af[i] = cvt8(lo, hi);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int n = j * 16 + cq, sw = (n >> 1) & 7;
                const unsigned char *row = Bs + n * 128 + 8 * (g & 1);
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                typedef __attribute__((address_space(3))) const volatile u32x2 lds_u32x2;
                const u32x2 lo = *(lds_u32x2 *)(row + ((4 * kk + (g >> 1)) ^ sw) * 16);
                const u32x2 hi = *(lds_u32x2 *)(row + ((4 * kk + 2 + (g >> 1)) ^ sw) * 16);
                const bf16x8 bf = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
#pragma unroll
                for (int i = 0; i < TMW; ++i) acc[i][j] = mma(af[i], bf, acc[i][j]);
            }
        }
    };
    f32x4_t xa[2][TMW][2], xb[2][TMW][2];
    // VM program order of a wave (A(i) = the A_LD frame loads of stage i, W(j) = the B_DMA DMA pieces of W stage j, W(j) exists
    // for j < nst only; A(nst) is a clamped re-load of the last stage whose registers are never consumed):
    //   prologue   W(0) .. W(D-2)  A(0)  W(D-1)
    //   stage i    A(i+1) | wait | barrier | W(i+D) | compute(i)
    // i.e. uniformly  ... A(i) W(i+D-1) A(i+1) W(i+D) ...  : at the wait of stage i everything up to and including A(i) must be
    // complete (W(i) is older than A(i) for D >= 2), and the only younger operations are W(i+D-1) -- if it exists -- and A(i+1).
    // (Round 2 issued the prologue as W(0) W(1) A(0) and waited vmcnt(A_LD + B_DMA) everywhere: in stage 0 the younger operations
    // were A(1) only, so the four youngest loads of A(0) could still be in flight when compute() converted them; the same at the
    // last stage, where no W stage follows A(nst-1).)
    static_assert(D >= 2, "W(i) must be older than A(i)");
#pragma unroll
    for (int s = 0; s < D - 1; ++s)
        if (s < nst) dir_issue_b<NW>(a, smem + s * C::B_BYTES, n0, stage_k(s), wave, lane);
    load_a(stage_k(0), xa);
    if (D - 1 < nst) dir_issue_b<NW>(a, smem + (D - 1) * C::B_BYTES, n0, stage_k(D - 1), wave, lane);
    auto wait_stage = [&](int i) {
        if (i + D - 1 < nst) wait_vm<C::A_LD + C::B_DMA>();     // younger than A(i): W(i+D-1), A(i+1)
        else wait_vm<C::A_LD>();                                // younger than A(i): A(i+1)
    };
    for (int s = 0; s < nst; s += 2) {
        load_a(stage_k(min(s + 1, nst - 1)), xb);
        wait_stage(s);
        barrier();
        if (s + D < nst) dir_issue_b<NW>(a, smem + ((s + D) % NS) * C::B_BYTES, n0, stage_k(s + D), wave, lane);
        compute(smem + (s % NS) * C::B_BYTES, xa);
        if (s + 1 >= nst) break;
        load_a(stage_k(min(s + 2, nst - 1)), xa);
        wait_stage(s + 1);
        barrier();
        if (s + 1 + D < nst) dir_issue_b<NW>(a, smem + ((s + 1 + D) % NS) * C::B_BYTES, n0, stage_k(s + 1 + D), wave, lane);
        compute(smem + ((s + 1) % NS) * C::B_BYTES, xb);
    }
    wait_vm<0>();                  // the clamped extra stage loads of the last round
    // epilogue: + bias, through LDS as fp32, one 16-row tile per wave per pass, 16-byte bf16 stores
    constexpr int LDC = C::BN + 4;
    float *Cs = reinterpret_cast<float *>(smem) + wave * 16 * LDC;
    // this lane's eight bias values, all loads in flight at once (read where they are used, under `a.bias ? ... : 0`, they
    // were 8 serialised L2 round trips per row tile: ~16 per workgroup lifetime)
    float bv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = 0.f;
    if (a.bias) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = a.bias[n0 + j * 16 + cq];
    }
#pragma unroll
    for (int i = 0; i < TMW; ++i) {
        barrier();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int lc = j * 16 + cq;
#pragma unroll
            for (int r = 0; r < 4; ++r) Cs[(4 * g + r) * LDC + lc] = acc[i][j][r] + bv[j];
        }
        barrier();
        for (int c = lane; c < 16 * (C::BN / 8); c += 64) {
            const int lr = c / (C::BN / 8), lc = (c % (C::BN / 8)) * 8;
            const int row = m0 + (wave * TMW + i) * 16 + lr;
            if (row < a.M) {
                float v[8];
                *reinterpret_cast<float4 *>(v) = *reinterpret_cast<const float4 *>(Cs + lr * LDC + lc);
                *reinterpret_cast<float4 *>(v + 4) = *reinterpret_cast<const float4 *>(Cs + lr * LDC + lc + 4);
                store16(a.Y + (int64_t)row * a.E + n0 + lc, v);
            }
        }
    }
}

template <int TMW, int NW, int NS>
int fwd_direct2_launch(const EmbFwdArgs &a, hipStream_t s) {
    using C = DirCfg<TMW, NW, NS>;
    const size_t ring = (size_t)NS * C::B_BYTES, scratch = (size_t)NW * 16 * (C::BN + 4) * 4;
    const size_t bytes = ring > scratch ? ring : scratch;
    auto kern = embed_fwd_direct2<TMW, NW, NS>;
    MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    ProfScope prof(s);
    hipLaunchKernelGGL(kern, dim3(a.E / 128, ceil_div(a.M, C::BM)), dim3(NW * 64), bytes, s, a);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

template <int TMW, int NW, int NS>
int fwd_direct_launch(const EmbFwdArgs &a, hipStream_t s) {
    using C = DirCfg<TMW, NW, NS>;
    const size_t ring = (size_t)NS * C::B_BYTES, scratch = (size_t)NW * 16 * (C::BN + 4) * 4;
    const size_t bytes = ring > scratch ? ring : scratch;
    auto kern = embed_fwd_direct<TMW, NW, NS>;
    MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    ProfScope prof(s);
    hipLaunchKernelGGL(kern, dim3(a.E / 128, ceil_div(a.M, C::BM)), dim3(NW * 64), bytes, s, a);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

// =================================================================================================================
// wgrad: tile 128 rows (e) x BKC columns (k of X), stage = 64 reduction rows m of dY (256 B rows) + of X (4*BKC B rows).
// 2 x BKC/64 waves, each a 64 x 64 sub-tile.  NS ring slots, NS - 1 stages in flight.
// =================================================================================================================
template <int BKC, int NS, int BMR_ = 64>
struct WgCfg {
    static constexpr int BE = 128, BMR = BMR_;
    static constexpr int NW = 2 * (BKC / 64);
    static constexpr int A_BYTES = BMR * BE * 2;         // 16 KiB
    static constexpr int B_ROW = BKC * 4;                // bytes per X row in the tile
    static constexpr int B_BYTES = BMR * B_ROW;          // 32 / 64 KiB
    static constexpr int STAGE = A_BYTES + B_BYTES;
    static constexpr int A_DMA = A_BYTES / 1024 / NW;
    static constexpr int B_DMA = B_BYTES / 1024 / NW;
    static constexpr int PER_STAGE = A_DMA + B_DMA;
    static constexpr int A_CH = BE / 8;                  // 16-byte chunks per dY row
    static constexpr int B_CH = B_ROW / 16;              // 16-byte chunks per X row (32 / 64)
    static_assert(A_DMA * NW * 1024 == A_BYTES && B_DMA * NW * 1024 == B_BYTES, "stage must split evenly over the waves");
};

struct EmbWgArgs {
    const bf16 *dY; const float *X; float *slabs;
    int M, K, E, rows_per_split;
    int xcd_remap;
};

template <int BKC, int NS, int BMR>
__device__ __forceinline__ void wg_issue(const EmbWgArgs &a, unsigned char *slot, int e0, int k0, int mrow, int mend,
                                         int wave, int lane) {
    using C = WgCfg<BKC, NS, BMR>;
#pragma unroll
    for (int i = 0; i < C::A_DMA; ++i) {              // dY: 4 rows of 256 B per wave-instruction
        const int inst = wave * C::A_DMA + i;
        const int r = inst * 4 + (lane >> 4), s = lane & 15;
        const int c = s ^ (2 * (r & 7));
        const int gm = min(mrow + r, mend - 1);
        dma16_tracked(a.dY + (int64_t)gm * a.E + e0 + c * 8, slot + inst * 1024);
    }
    unsigned char *bs = slot + C::A_BYTES;
    constexpr int RPI = 64 / C::B_CH == 0 ? 1 : 1024 / C::B_ROW;    // X rows per wave-instruction (2 or 1)
#pragma unroll
    for (int i = 0; i < C::B_DMA; ++i) {
        const int inst = wave * C::B_DMA + i;
        const int r = inst * RPI + lane / C::B_CH, s = lane % C::B_CH;
        const int c = s ^ (((r >> 3) & 1) << 2);          // rows 8 apart land 16 floats (= 16 banks) apart
        const int gm = min(mrow + r, mend - 1);
        dma16_tracked(a.X + (int64_t)gm * a.K + k0 + c * 4, bs + inst * 1024);
    }
}

template <int BKC, int NS, int BMR>
__global__ __launch_bounds__(2 * (BKC / 64) * 64, BMR == 32 ? 4 : 1) void embed_wgrad_dma(const EmbWgArgs a) {
    using C = WgCfg<BKC, NS, BMR>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TM = 4, TN = 4, D = NS - 1;
    constexpr int WN = BKC / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    // XCD-aware placement: the K / BKC column tiles of one row split all re-read the same d_emb rows; within 8 * T consecutive
    // workgroups (dispatch order, x fastest, dealt round-robin over the 8 XCDs) XCD k hosts all T tiles of split 8 * group + k
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    {
        const int T = gridDim.x * gridDim.y, lin = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, G = 8 * T;
        if (a.xcd_remap && T > 1 && lin < (int)(T * gridDim.z) / G * G) {
            const int t = (lin % G) / 8;
            bz = (lin / G) * 8 + lin % 8; bx = t % gridDim.x; by = t / gridDim.x;
        }
    }
    const int k0 = bx * BKC, e0 = by * C::BE;
    const int mb = bz * a.rows_per_split, me = min(a.M, mb + a.rows_per_split);
    const int nst = (me - mb + C::BMR - 1) / C::BMR;
    const int g = lane >> 4, cq = lane & 15, q = cq >> 2, p = cq & 3;

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s = 0; s < D; ++s)
        if (s < nst) wg_issue<BKC, NS, BMR>(a, smem + s * C::STAGE, e0, k0, mb + s * C::BMR, me, wave, lane);
    for (int s = 0; s < nst; ++s) {
        if (s + D - 1 < nst) wait_vm<C::PER_STAGE * (D - 1)>();
        else wait_vm<0>();
        barrier();
        if (s + D < nst) wg_issue<BKC, NS, BMR>(a, smem + ((s + D) % NS) * C::STAGE, e0, k0, mb + (s + D) * C::BMR, me, wave, lane);
        const unsigned char *As = smem + (s % NS) * C::STAGE, *Bs = As + C::A_BYTES;
        const int valid = min(C::BMR, me - (mb + s * C::BMR));     // rows of this stage inside the split
#pragma unroll
        for (int kk = 0; kk < BMR / 32; ++kk) {
            // k slots 0..3 = rows kk*32 + 8g + 0..3, slots 4..7 = rows kk*32 + 8g + 4..7 (both operands)
            const int mr = kk * 32 + 8 * g;
            bf16x8 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                // A[e][m] from the natural [m][e] image: transposed read of 4 rows x 16 e (two per fragment)
                const int ecol = wm * 64 + i * 16 + 4 * p;                 // this lane supplies e columns ecol..ecol+3
                s16x4 lo, hi;
                {
                    const int r = mr + q;
                    const int c = (ecol >> 3) ^ (2 * (r & 7));
                    lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4 *)(As + r * 256 + c * 16 + (ecol & 7) * 2));
                }
                {
                    const int r = mr + 4 + q;
                    const int c = (ecol >> 3) ^ (2 * (r & 7));
                    hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4 *)(As + r * 256 + c * 16 + (ecol & 7) * 2));
                }
                struct { s16x4 a, b; } pr = {lo, hi};
                af[i] = __builtin_bit_cast(bf16x8, pr);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = wn * 64 + j * 16 + cq;                       // output column (k of X) of this lane
                float v[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const int r = mr + t;
                    const int c = (n >> 2) ^ (((r >> 3) & 1) << 2);
                    const float x = *reinterpret_cast<const float *>(Bs + r * C::B_ROW + c * 16 + (n & 3) * 4);
                    v[t] = r < valid ? x : 0.f;                            // rows past the split end repeat the last row
                }
                bf[j] = cvt8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]));
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mma(af[i], bf[j], acc[i][j]);
        }
    }
    // slab[z][e][k] fp32 straight from the accumulator layout (column = k, rows = e)
    float *out = a.slabs + (int64_t)bz * a.E * a.K;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = e0 + wm * 64 + i * 16 + 4 * g + r;
                out[(int64_t)e * a.K + k0 + wn * 64 + j * 16 + cq] = acc[i][j][r];
            }
}

bool wg_wide(int K) {
    static const int variant = getenv("MIVIT_EMBED_WGRAD_VARIANT") ? atoi(getenv("MIVIT_EMBED_WGRAD_VARIANT")) : 1;
    return variant == 1 && K % 256 == 0;
}

int wg_splits(int M, int K, int E) {
    const long tiles = (long)(K / (wg_wide(K) ? 256 : 128)) * (E / 128 > 0 ? E / 128 : 1);
    static const int target = getenv("MIVIT_EMBED_WGRAD_BLOCKS") ? atoi(getenv("MIVIT_EMBED_WGRAD_BLOCKS")) : 512;
    long s = (target + tiles - 1) / tiles;         // two resident workgroups per CU
    const long maxs = (M + 511) / 512;
    if (s > maxs) s = maxs;
    if (s < 1) s = 1;
    return (int)s;
}

template <int BM, int NS>
int fwd_dma_launch(const EmbFwdArgs &a, hipStream_t s) {
    using C = FwdCfg<BM, NS>;
    const size_t bytes = (size_t)NS * C::STAGE;
    auto kern = embed_fwd_dma<BM, NS>;
    MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    ProfScope prof(s);
    hipLaunchKernelGGL(kern, dim3(a.E / 128, ceil_div(a.M, BM)), dim3(C::NW * 64), bytes, s, a);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// forward tiling, selectable for A/B runs and so that the tests reach every launcher branch at small sizes:
// MIVIT_EMBED_FWD_VARIANT / mivit_embed_set_variant (0 = by problem size)
static int g_embed_variant = getenv("MIVIT_EMBED_FWD_VARIANT") ? atoi(getenv("MIVIT_EMBED_FWD_VARIANT")) : 0;
extern "C" int mivit_embed_set_variant(int v) {
    const int old = g_embed_variant; g_embed_variant = v;
    if (v != old) graph_switch_changed();          // captured launch sequences made under the old value start over
    return old;
}

bool embed_dma_supported(int dtype, int M, int K, int E) {
    return dtype == MIVIT_ELEM_DTYPE && E % 128 == 0 && K % 128 == 0 && K >= 256 && M >= 128;
}

int launch_embed_fwd_dma(const float *X, const void *W_bf16, const float *bias, void *Y, int M, int K, int E,
                         hipStream_t s) {
    MIVIT_CHECK(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(W_bf16) | reinterpret_cast<uintptr_t>(Y)) & 15) == 0,
                "embed_fwd_dma: operands must be 16-byte aligned");
    EmbFwdArgs a = {X, static_cast<const bf16 *>(W_bf16), bias, static_cast<bf16 *>(Y), M, K, E, 0};
    // measured (c1, batch 16384): 0 -> 4.78 TB/s, 1 -> 5.06, 3 -> 5.09, 5..13 -> 5.00-5.03, 17 -> 5.09, 21 -> 5.03
    static const int kstag = getenv("MIVIT_EMBED_KSTAG") ? atoi(getenv("MIVIT_EMBED_KSTAG")) : 17;
    a.kstag = kstag;
    const int variant = g_embed_variant;
    if (variant == 2) return fwd_dma_launch<128, 3>(a, s);
    if (variant == 1) return fwd_dma_launch<256, 2>(a, s);     // LDS-DMA staging of the frames (first design, kept for A/B runs)
    switch (variant) {
        case 3: return fwd_direct_launch<2, 4, 3>(a, s);
        case 14: return fwd_direct2_launch<2, 4, 3>(a, s);
        case 4: return fwd_direct_launch<1, 4, 2>(a, s);
        case 5: return fwd_direct_launch<1, 8, 3>(a, s);
        case 6: return fwd_direct_launch<1, 8, 2>(a, s);
        case 7: return fwd_direct_launch<2, 4, 2>(a, s);
        case 8: return fwd_direct_launch<1, 4, 3>(a, s);
        case 15: return fwd_direct_launch<1, 2, 3>(a, s);
        case 13: {
            const size_t bytes = (size_t)F32Cfg::NS * F32Cfg::STAGE;
            MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(embed_fwd_dma32), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
            ProfScope prof(s);
            hipLaunchKernelGGL(embed_fwd_dma32, dim3(a.E / 128, ceil_div(a.M, F32Cfg::BM)), dim3(512), bytes, s, a);
            MIVIT_LAUNCH_CHECK();
            return 0;
        }
        default:
            // small problems: shrink the row tile until the grid covers the chip (a 128-row tile gives M / 128 workgroups)
            if ((long)ceil_div(a.M, 128) * (a.E / 128) >= 512) return fwd_direct2_launch<2, 4, 3>(a, s);
            if ((long)ceil_div(a.M, 64) * (a.E / 128) >= 512) return fwd_direct_launch<1, 4, 3>(a, s);
            return fwd_direct_launch<1, 2, 3>(a, s);
    }
}

size_t embed_wgrad_dma_ws_bytes(int M, int K, int E) { return (size_t)wg_splits(M, K, E) * E * K * sizeof(float); }

template <int BKC, int NS, int BMR>
static int wg_dma_launch(EmbWgArgs a, int nz, hipStream_t s) {
    using C = WgCfg<BKC, NS, BMR>;
    const size_t bytes = (size_t)NS * C::STAGE;
    auto kern = embed_wgrad_dma<BKC, NS, BMR>;
    MIVIT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    ProfScope prof(s);
    hipLaunchKernelGGL(kern, dim3(a.K / BKC, a.E / 128, nz), dim3(C::NW * 64), bytes, s, a);
    MIVIT_LAUNCH_CHECK();
    return 0;
}

int launch_embed_wgrad_dma(const void *dY_bf16, const float *X, float *dW, int M, int K, int E, void *ws, size_t ws_bytes,
                           hipStream_t s) {
    MIVIT_CHECK(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(dY_bf16) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
                "embed_wgrad_dma: operands must be 16-byte aligned");
    const int splits = wg_splits(M, K, E);
    MIVIT_CHECK(ws_bytes >= embed_wgrad_dma_ws_bytes(M, K, E), "embed_wgrad_dma: workspace too small");
    int rps = ceil_div(M, splits);
    rps = (rps + 63) / 64 * 64;
    const int nz = ceil_div(M, rps);
    static const int remap = getenv("MIVIT_XCD_REMAP") ? atoi(getenv("MIVIT_XCD_REMAP")) : 1;
    EmbWgArgs a = {static_cast<const bf16 *>(dY_bf16), X, static_cast<float *>(ws), M, K, E, rps, remap};
    // 32-row stages: 80 KB ring and <= 128 registers -> two workgroups (16 waves) per CU; measured 1.67 -> 1.39 ms/step
    // against the 64-row / 160 KB / one-workgroup point (MIVIT_EMBED_WGRAD_CFG=2 selects that one)
    static const int variant = getenv("MIVIT_EMBED_WGRAD_CFG") ? atoi(getenv("MIVIT_EMBED_WGRAD_CFG")) : 1;
    int rc;
    if (!wg_wide(K)) rc = wg_dma_launch<128, 3, 64>(a, nz, s);
    else if (variant == 2) rc = wg_dma_launch<256, 2, 64>(a, nz, s);
    else rc = wg_dma_launch<256, 2, 32>(a, nz, s);
    if (rc) return rc;
    return launch_slab_reduce(static_cast<const float *>(ws), nz, (int64_t)E * K, dW, 0, s);
}

// operator-level C-ABI (include/mivit_hip.h): the fp16 build exports the same entries suffixed _f16 (elem.h)
extern "C" int mivit_embed_fwd_bf16(const float *x, const void *W_bf16, const float *bias, int M, int K, int E,
                                    void *y_bf16, void *stream) {
    MIVIT_CHECK(x && W_bf16 && y_bf16, "embed_fwd_bf16: null pointer");
    if (!embed_dma_supported(MIVIT_ELEM_DTYPE, M, K, E)) { mivit_set_error("embed_fwd_bf16: unsupported shape"); return 3; }
    prof_set_tag(MIVIT_PROF_OP);
    return launch_embed_fwd_dma(x, W_bf16, bias, y_bf16, M, K, E, static_cast<hipStream_t>(stream));
}
extern "C" size_t mivit_embed_wgrad_bf16_workspace_bytes(int M, int K, int E) {
    return embed_dma_supported(MIVIT_ELEM_DTYPE, M, K, E) ? embed_wgrad_dma_ws_bytes(M, K, E) : 0;
}
extern "C" int mivit_embed_wgrad_bf16(const void *dy_bf16, const float *x, int M, int K, int E, float *dW,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    MIVIT_CHECK(dy_bf16 && x && dW && workspace, "embed_wgrad_bf16: null pointer");
    if (!embed_dma_supported(MIVIT_ELEM_DTYPE, M, K, E)) { mivit_set_error("embed_wgrad_bf16: unsupported shape"); return 3; }
    prof_set_tag(MIVIT_PROF_OP);
    return launch_embed_wgrad_dma(dy_bf16, x, dW, M, K, E, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
