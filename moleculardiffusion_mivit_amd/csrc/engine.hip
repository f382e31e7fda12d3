// Model-level engine: GeneralTransformer.forward and its backward as a fixed sequence of HIP launches
// (reference helpers/models.py:328-361 orchestration, :136-141 Transformer, :97-108 post-norm encoder layer,
// :33-59 attention, :72-77 feed-forward, :268-276 MLP head).  Host code only: every arithmetic step is one of
// the kernels in gemm.hip / norm.hip / attention.hip / misc.hip.  The engine owns no device memory: the caller
// passes the parameter arena, the gradient arena and one workspace whose layout is computed here.
#include "common.h"
#include "slab_defer.h"
#include <atomic>
#include <algorithm>

#include <string>
#include <vector>

// fused encoder-layer blocks (fused_fwd.hip / fused_bwd.hip): one set of externals per element type and layer width (elem.h:
// the two units are compiled as is, with -DMIVIT_ELEM_F16, with -DMIVIT_WIDTH64 and with both)
#define MIVIT_FUSED_DECLS(SFX)                                                                                                     \
    bool fused_layer_supported##SFX(int dtype, int E, int F, int H, int S);                                                        \
    int launch_attn_block_fwd##SFX(const void *nin, const float *gin, const float *bin, const void *Wqkv, const float *bqkv,       \
                                   const void *Wo, const float *bo, const float *gout, const float *bout, int B, int S, void *ctx, \
                                   void *nout, float *rstd, void *xout, void *zout, float *mean, void *qkvout, bool q1,            \
                                   hipStream_t s);                                                                                 \
    int launch_mlp_block_fwd##SFX(const void *nin, const float *gin, const float *bin, const void *W1, const float *b1,            \
                                  const void *W2, const float *b2, const float *gout, const float *bout, int M, int act,           \
                                  void *nout, float *rstd, void *xout, void *zout, float *mean, void *hout, void *uout,            \
                                  hipStream_t s);                                                                                  \
    size_t mlp_block_bwd_ws_bytes##SFX(int M);                                                                                     \
    size_t attn_out_bwd_ws_bytes##SFX(int M);                                                                                      \
    int launch_attn_out_bwd##SFX(const void *dy, const void *n1, const float *rstd1, const float *gamma1, const void *ctx,         \
                                 const void *Wo, int M, int live_S, void *dz1, void *dctx, float *dWo, float *dbo,                 \
                                 float *dgamma1, float *dbeta1, void *ws, size_t ws_bytes, hipStream_t s);                         \
    int launch_mlp_block_bwd##SFX(const void *dy, const void *n2, const float *rstd2, const float *gamma2, const void *n1,         \
                                  const float *gamma1, const float *beta1, const void *W1, const float *b1, const void *W2, int M, \
                                  int act, void *dx1, float *dW1, float *db1, float *dW2, float *db2, float *dgamma2,              \
                                  float *dbeta2, void *ws, size_t ws_bytes, hipStream_t s);                                        \
    size_t qkv_bwd_ws_bytes##SFX(int M);                                                                                           \
    int launch_qkv_bwd##SFX(const void *dqkv, const void *x, const void *Wqkv, const void *res, int M, void *dx, float *dW,        \
                            float *db, const float *fix_gamma, const float *fix_beta, void *ws, size_t ws_bytes, hipStream_t s);
MIVIT_FUSED_DECLS()
MIVIT_FUSED_DECLS(_f16)
MIVIT_FUSED_DECLS(_w64)
MIVIT_FUSED_DECLS(_w64_f16)
#undef MIVIT_FUSED_DECLS

struct FusedOps {
    decltype(&fused_layer_supported) ok;
    decltype(&launch_attn_block_fwd) attn_fwd;
    decltype(&launch_mlp_block_fwd) mlp_fwd;
    decltype(&launch_mlp_block_bwd) mlp_bwd;
    decltype(&launch_attn_out_bwd) attn_out_bwd;
    decltype(&mlp_block_bwd_ws_bytes) mlp_bwd_ws;
    decltype(&attn_out_bwd_ws_bytes) attn_out_bwd_ws;
    decltype(&launch_qkv_bwd) qkv_bwd;
    decltype(&qkv_bwd_ws_bytes) qkv_bwd_ws;
};
#define MIVIT_FUSED_TABLE(SFX)                                                                                                \
    {fused_layer_supported##SFX, launch_attn_block_fwd##SFX, launch_mlp_block_fwd##SFX, launch_mlp_block_bwd##SFX,            \
     launch_attn_out_bwd##SFX, mlp_block_bwd_ws_bytes##SFX, attn_out_bwd_ws_bytes##SFX, launch_qkv_bwd##SFX, qkv_bwd_ws_bytes##SFX}
static const FusedOps kFusedBf16 = MIVIT_FUSED_TABLE(), kFusedF16 = MIVIT_FUSED_TABLE(_f16), kFusedBf16W64 = MIVIT_FUSED_TABLE(_w64),
                      kFusedF16W64 = MIVIT_FUSED_TABLE(_w64_f16);
#undef MIVIT_FUSED_TABLE
// (MIVIT_NO_FUSED_W64: the reference's shipped width back on the per-operator streaming path -- A/B measurements)
static const FusedOps *fused_ops(int dtype, int E) {
    static const bool f16_off = getenv("MIVIT_NO_F16_STREAM") != nullptr, w64_off = getenv("MIVIT_NO_FUSED_W64") != nullptr;
    if (E == 64 && w64_off) return nullptr;
    if (dtype == MIVIT_BF16) return E == 64 ? &kFusedBf16W64 : &kFusedBf16;
    if (dtype == MIVIT_F16 && !f16_off) return E == 64 ? &kFusedF16W64 : &kFusedF16;
    return nullptr;
}
// Readout-row pruning: under the regression-token readout the head reads B rows of the last layer's output.
//   1 (default)  what leaves every result as it was: the last feed-forward block's forward on those B rows, the attention core's
//                backward on the one query row per sequence that carries a gradient; every weight-gradient sum as before.  And
//                the readout QUERY: the last attention block's query side for row tile 0 only, its LayerNorm-1 / out-projection
//                and attention-core backward reading the readout rows only where every other row is an exact zero (rq_parts)
//   3            mode 1 without the readout-query part: the launches mode 1 made before it (A/B measurements, tests)
//   2            also the feed-forward block's and LayerNorm-1 / out-projection's backward on B rows: the last layer's fc1 /
//                fc2 / norm2 / out_proj / norm1 gradients then sum the same fp32 terms in another order (MIVIT_READOUT_ROWS=2)
//   0            every row (MIVIT_NO_READOUT_ROWS, mivit_set_readout_rows(0): A/B measurements, parity tests)
static int g_readout_rows = getenv("MIVIT_NO_READOUT_ROWS") ? 0 : (getenv("MIVIT_READOUT_ROWS") ? atoi(getenv("MIVIT_READOUT_ROWS")) : 1);
extern "C" int mivit_set_readout_rows(int on) { const int old = g_readout_rows; g_readout_rows = on; return old; }
// The parts of mode 1's readout query, MIVIT_READOUT_QUERY_PARTS = their bit mask (read once; A/B measurements of single parts):
//   1  attn_block_fwd: query side for row tile 0 only (fused_fwd.hip, Q1).  It leaves q, ctx and rstd1 behind tile 0 unwritten,
//      so with it attn_bwd_fast2 reads of q only the rows that carry a gradient (q_lean), and it needs part 2
//   2  attn_out_bwd: d(x1) / n1 / rstd1 / ctx read and d(ctx) written in the readout rows only
// The q|k|v backward is unchanged and reads every row: d(z1) and dq keep their zero rows.
static int rq_parts() {
    static const int parts = [] {
        const char *e = getenv("MIVIT_READOUT_QUERY_PARTS");
        int m = e ? atoi(e) & 3 : 3;
        if (!(m & 2)) m &= ~1;
        return m;
    }();
    return parts;
}

static bool fused_ok(int dtype, int E, int F, int H, int S) {
    const FusedOps *f = fused_ops(dtype, E);
    return f && f->ok(dtype, E, F, H, S);
}

struct ParamInfo {
    std::string name;
    int64_t offset, numel;
};

struct LayerParams {
    int64_t qkv_w, qkv_b, out_w, out_b, n1_w, n1_b, fc1_w, fc1_b, fc2_w, fc2_b, n2_w, n2_b;
};

struct mivit_plan {
    mivit_config c;
    std::vector<ParamInfo> params;
    std::vector<std::pair<int64_t, int64_t>> stages;
    int64_t arena;
    // offsets (floats) into the arena
    int64_t tn_w, tn_b, fp0_w, fp0_b, fp2_w, fp2_b, h0_w, h0_b, h3_w, h3_b;
    std::vector<LayerParams> layers;
    int64_t reg, pos, n0_w, n0_b, emb_w, emb_b;
    int head_in;
    uint64_t uid;       // unique per created plan: hipGraph keys use it, never the pointer (a freed plan's address can be reused)
};

namespace {

constexpr int MAX_TOKENS = 128;   // helpers/models.py:8

int64_t add_param(mivit_plan *p, const std::string &name, int64_t numel, bool align = true) {
    // 32-byte aligned fp32 tensors = 16-byte aligned in the bf16 shadow copy (k/v follow q unpadded: one operand)
    if (align) p->arena = (p->arena + 7) / 8 * 8;
    const int64_t off = p->arena;
    p->params.push_back({name, off, numel});
    p->arena += numel;
    return off;
}

void add_feature_projector(mivit_plan *p) {
    const int E = p->c.embed_dim, G = p->c.global_feature_dim;
    p->fp0_w = add_param(p, "feature_projector.0.weight", (int64_t)E * G);
    p->fp0_b = add_param(p, "feature_projector.0.bias", E);
    p->fp2_w = add_param(p, "feature_projector.2.weight", (int64_t)E * E);
    p->fp2_b = add_param(p, "feature_projector.2.bias", E);
}

struct Ws {
    size_t total;
    size_t wsh;          // bf16 shadow of the parameter arena (bf16 mode), refreshed by every forward
    size_t emb, mean0, rstd0, x0;
    struct L { size_t qkv, ctx, z1, x1, h, u, z2, x2, mean1, rstd1, mean2, rstd2; };
    std::vector<L> layer;
    size_t xF, meanF, rstdF, pooled, fp_h, fp_out, head_in, hh;
    size_t xL;           // fused layer blocks: x = gamma * xhat + beta of the LAST layer (input of the final norm)
    // readout rows (fused blocks, regression token, S > 1): row b * S of the last layer's z1 gathered to [B,E]; that layer's
    // compact z2 / rstd2 / xL use the first B rows of the full regions.  Backward: the same gather of rstd1 and ctx, compact
    // d(z1) and d(ctx)
    size_t z1c, rstd1c, ctxc, dz1c, dctxc;
    size_t z2c, rstd2c, xLc;          // mode 1: the compact block's outputs before they are scattered to rows b * S of the full regions
    // backward temporaries
    size_t dout_t, d_hh, d_head_in, d_pool_c, d_fp_h, dxa, dxb, dF, dctx, dqkv, wgrad, ln, colsum;
    size_t wgrad_bytes, ln_bytes, colsum_bytes;
};

Ws make_ws(const mivit_plan *p, int B, int T, bool bwd) {
    const mivit_config &c = p->c;
    const size_t ts = dtype_size(c.dtype);
    const int E = c.embed_dim, F = c.hidden_dim, L = c.num_layers;
    const int S = T + (c.use_regression_token ? 1 : 0);
    const size_t M = (size_t)B * S, Mt = (size_t)B * T;
    Ws w = {};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes, 256); return o; };
    w.wsh = c.dtype != MIVIT_F32 ? take((size_t)p->arena * 2) : 0;
    w.emb = take(Mt * E * ts); w.mean0 = take(Mt * 4); w.rstd0 = take(Mt * 4);
    w.x0 = take(M * E * ts);
    const int nsets = bwd ? L : 1;
    const bool fused = L > 0 && fused_ok(c.dtype, E, F, c.num_heads, S);
    for (int l = 0; l < nsets; ++l) {
        Ws::L s;
        if (fused) {
            // fused layer blocks: z1 / z2 hold the NORMALISED sub-layer outputs (xhat, bf16), rstd1 / rstd2 their 1/std;
            // q|k|v and h are kept only for the backward; no pre-norm sums, no means, no x copies
            s.qkv = bwd ? take(M * 3 * E * ts) : 0; s.ctx = take(M * E * ts); s.z1 = take(M * E * ts); s.x1 = 0;
            s.h = 0; s.u = 0;
            s.z2 = take(M * E * ts); s.x2 = 0;
            s.mean1 = s.mean2 = 0; s.rstd1 = take(M * 4); s.rstd2 = take(M * 4);
        } else {
            s.qkv = take(M * 3 * E * ts); s.ctx = take(M * E * ts); s.z1 = take(M * E * ts); s.x1 = take(M * E * ts);
            s.h = take(M * F * ts); s.u = c.activation == MIVIT_ACT_GELU ? take(M * F * ts) : 0;
            s.z2 = take(M * E * ts); s.x2 = take(M * E * ts);
            s.mean1 = take(M * 4); s.rstd1 = take(M * 4); s.mean2 = take(M * 4); s.rstd2 = take(M * 4);
        }
        w.layer.push_back(s);
    }
    for (int l = nsets; l < L; ++l) w.layer.push_back(w.layer[0]);
    w.xL = fused ? take(M * E * ts) : 0;
    const bool rows = fused && c.use_regression_token && S > 1;
    w.z1c = rows ? take((size_t)B * E * ts) : 0;
    if (rows) { w.z2c = take((size_t)B * E * ts); w.rstd2c = take((size_t)B * 4); w.xLc = take((size_t)B * E * ts); }
    w.xF = c.use_regression_token ? 0 : take(M * E * ts);
    w.meanF = take(M * 4); w.rstdF = take(M * 4);
    w.pooled = take((size_t)B * E * ts);
    w.fp_h = take((size_t)B * E * ts); w.fp_out = take((size_t)B * E * ts);
    w.head_in = take((size_t)B * 2 * E * ts);
    w.hh = take((size_t)B * c.head_hidden * ts);
    if (bwd) {
        w.dout_t = take((size_t)B * c.output_dim * ts);
        w.d_hh = take((size_t)B * c.head_hidden * ts);
        w.d_head_in = take((size_t)B * 2 * E * ts);
        w.d_pool_c = take((size_t)B * E * ts);
        w.d_fp_h = take((size_t)B * E * ts);
        w.dxa = take(M * E * ts); w.dxb = take(M * E * ts);
        w.dF = take(M * F * ts); w.dctx = take(M * E * ts); w.dqkv = take(M * 3 * E * ts);
        if (rows) {
            w.rstd1c = take((size_t)B * 4); w.ctxc = take((size_t)B * E * ts);
            w.dz1c = take((size_t)B * E * ts); w.dctxc = take((size_t)B * E * ts);
        }
        size_t wg = 0;
        auto mx = [&](int m, int n, int k) {
            size_t b = linear_wgrad_ws_bytes(m, n, k);
            // (the bf16 and f16 builds of the weight-gradient kernels size their workspaces identically)
            if (c.dtype != MIVIT_F32 && n % 128 == 0 && k % 128 == 0 && m >= 256) b += wgrad_dma_ws_bytes(m, n, k);
            if (c.dtype != MIVIT_F32 && m >= 256) b = std::max(b, wgrad_small_ws_bytes(m, n, k));
            if (c.dtype != MIVIT_F32 && m >= 256) b = std::max(b, embed_small_wgrad_ws_bytes(m, n, k));      // (the embedding's shape only)
            if (b > wg) wg = b;
        };
        mx((int)M, 3 * E, E); mx((int)M, E, E); mx((int)M, F, E); mx((int)M, E, F);
        if (fused) {
            const FusedOps *fo = fused_ops(c.dtype, E);
            // (one region each: their slab reductions are deferred to one launch per layer, so the three slab sets coexist)
            wg = std::max(wg, fo->mlp_bwd_ws((int)M) + fo->attn_out_bwd_ws((int)M) + fo->qkv_bwd_ws((int)M));
        }
        if (c.embedding != MIVIT_EMBED_EXTERNAL) {
            mx((int)Mt, E, c.patch_size * c.patch_size);
            if ((c.dtype == MIVIT_F16 ? embed_dma_supported_f16 : embed_dma_supported)(c.dtype, (int)Mt, c.patch_size * c.patch_size, E)) {
                const size_t b = embed_wgrad_dma_ws_bytes((int)Mt, c.patch_size * c.patch_size, E);      // (same for both element types)
                if (b > wg) wg = b;
            }
        }
        mx(B, c.head_hidden, p->head_in); mx(B, c.output_dim, c.head_hidden);
        if (c.fusion != MIVIT_FUSION_NONE) { mx(B, E, E); mx(B, E, c.global_feature_dim); }
        w.wgrad_bytes = wg; w.wgrad = take(wg);
        w.ln_bytes = layernorm_bwd_ws_bytes((int)M, E); w.ln = take(w.ln_bytes);
        w.colsum_bytes = batch_colsum_ws_bytes(B, S, E); w.colsum = take(w.colsum_bytes);
    }
    w.total = off;
    return w;
}

inline void *at(void *base, size_t off) { return static_cast<char *>(base) + off; }
inline const void *at(const void *base, size_t off) { return static_cast<const char *>(base) + off; }
// pointer `cols` elements into a row of a T matrix
inline void *col_ptr(void *p, size_t cols, int dtype) { return static_cast<char *>(p) + cols * dtype_size(dtype); }

#define RC(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

// The streaming kernels exist once per 16-bit element type (elem.h: each unit is compiled for bf16 and, with
// -DMIVIT_ELEM_F16, for IEEE half): the plan's dtype picks the set.  fp32 (parity mode) has none: general kernels.
struct StreamOps {
    decltype(&rowstream_supported) rowstream_ok;
    decltype(&wavestream_supported) wavestream_ok;
    decltype(&launch_rowstream) rowstream;
    decltype(&wgrad_dma_supported) wgrad_dma_ok;
    decltype(&wgrad_dma_ws_bytes) wgrad_dma_ws;
    decltype(&launch_wgrad_dma) wgrad_dma;
    decltype(&wgrad_small_supported) wgrad_small_ok;
    decltype(&wgrad_small_ws_bytes) wgrad_small_ws;
    decltype(&launch_wgrad_small) wgrad_small;
    decltype(&embed_dma_supported) embed_ok;
    decltype(&launch_embed_fwd_dma) embed_fwd;
    decltype(&embed_wgrad_dma_ws_bytes) embed_wgrad_ws;
    decltype(&launch_embed_wgrad_dma) embed_wgrad;
    decltype(&embed_small_fwd_supported) embed_small_fwd_ok;          // small frames (any row length <= 256 pixels)
    decltype(&launch_embed_small_fwd) embed_small_fwd;
    decltype(&embed_small_wgrad_supported) embed_small_wgrad_ok;
    decltype(&embed_small_wgrad_ws_bytes) embed_small_wgrad_ws;
    decltype(&launch_embed_small_wgrad) embed_small_wgrad;
};
static const StreamOps kStreamBf16 = {rowstream_supported, wavestream_supported, launch_rowstream, wgrad_dma_supported, wgrad_dma_ws_bytes,
                                      launch_wgrad_dma, wgrad_small_supported, wgrad_small_ws_bytes, launch_wgrad_small,
                                      embed_dma_supported, launch_embed_fwd_dma, embed_wgrad_dma_ws_bytes, launch_embed_wgrad_dma,
                                      embed_small_fwd_supported, launch_embed_small_fwd, embed_small_wgrad_supported,
                                      embed_small_wgrad_ws_bytes, launch_embed_small_wgrad};
static const StreamOps kStreamF16 = {rowstream_supported_f16, wavestream_supported_f16, launch_rowstream_f16, wgrad_dma_supported_f16,
                                     wgrad_dma_ws_bytes_f16, launch_wgrad_dma_f16, wgrad_small_supported_f16, wgrad_small_ws_bytes_f16,
                                     launch_wgrad_small_f16, embed_dma_supported_f16, launch_embed_fwd_dma_f16,
                                     embed_wgrad_dma_ws_bytes_f16, launch_embed_wgrad_dma_f16, embed_small_fwd_supported_f16,
                                     launch_embed_small_fwd_f16, embed_small_wgrad_supported_f16, embed_small_wgrad_ws_bytes_f16,
                                     launch_embed_small_wgrad_f16};
static const StreamOps *stream_ops(int dtype) {
    static const bool f16_off = getenv("MIVIT_NO_F16_STREAM") != nullptr;        // (A/B: fp16 on the general kernels, as in rounds 1-2)
    return dtype == MIVIT_BF16 ? &kStreamBf16 : (dtype == MIVIT_F16 && !f16_off ? &kStreamF16 : nullptr);
}
// row-stream (DMA ring) or wave-stream kernels: launch_rowstream picks between the two families
static bool stream_gemm_supported(const StreamOps *so, int M, int N, int K, bool dgrad, int64_t lda, int64_t ldw, const void *A, const void *W) {
    return so && (so->rowstream_ok(M, N, K, dgrad, lda, ldw, A, W) || so->wavestream_ok(M, N, K, dgrad, lda, ldw, A, W));
}

int lin_fwd(int dtype, const void *x, int x_f32, int64_t ldx, const void *W, const float *b, int M, int N, int K,
            int act, const void *resid, int64_t ldr, void *y, int64_t ldy, void *pre, int y_f32, hipStream_t s) {
    const StreamOps *so = stream_ops(dtype);
    if (!x_f32 && !y_f32 && stream_gemm_supported(so, M, N, K, false, ldx, K, x, W) &&
        (!resid || ldr % 8 == 0) && ldy % 8 == 0) {
        prof_set_tag(MIVIT_PROF_LINEAR_FWD);
        return so->rowstream(false, x, ldx, W, K, M, N, K, b, act, nullptr, 0, 0, resid, ldr, y, ldy, pre, nullptr,
                                nullptr, nullptr, 0, nullptr, nullptr, s);
    }
    if (dtype == MIVIT_BF16 && !x_f32 && !y_f32 && gemm_dma_supported(M, N, K, false) && ldx % 8 == 0 && ldy % 8 == 0 &&
        (!resid || ldr % 8 == 0) && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(y) |
                                      reinterpret_cast<uintptr_t>(resid) | reinterpret_cast<uintptr_t>(pre)) & 15) == 0) {
        prof_set_tag(MIVIT_PROF_LINEAR_FWD);
        return launch_gemm_dma_fwd(x, ldx, W, b, M, N, K, act, resid, ldr, y, ldy, pre, s);
    }
    if (so && x_f32 && !y_f32 && ldx == K && ldy == N && act == MIVIT_ACT_NONE && !resid && !pre &&
        so->embed_small_fwd_ok(M, K, N, x, y)) {          // the linear embedding of small frames (fp32 rows of any length)
        prof_set_tag(MIVIT_PROF_EMBED_FWD);
        return so->embed_small_fwd(static_cast<const float *>(x), W, b, y, M, K, N, s);
    }
    LinearFwdArgs a = {};
    a.dtype = dtype; a.x = x; a.x_is_f32 = x_f32 || dtype == MIVIT_F32; a.ldx = ldx; a.W = W;
    a.w_is_bf16 = dtype != MIVIT_F32; a.bias = b;
    a.M = M; a.N = N; a.K = K; a.act = act; a.resid = resid; a.ldr = ldr; a.y = y; a.ldy = ldy; a.y_preact = pre;
    a.y_is_f32 = y_f32;
    prof_set_tag(x_f32 && K > 1024 ? MIVIT_PROF_EMBED_FWD : MIVIT_PROF_LINEAR_FWD);
    return launch_linear_fwd(a, s);
}
int lin_dgrad(int dtype, const void *dy, int64_t lddy, const void *W, int M, int N, int K, int act, const void *saved,
              int64_t lds, const void *dres, int64_t lddr, void *dx, int64_t lddx, int dx_f32, hipStream_t s) {
    const StreamOps *so = stream_ops(dtype);
    if (!dx_f32 && stream_gemm_supported(so, M, K, N, true, lddy, K, dy, W) && lddx % 8 == 0 &&
        (!dres || lddr % 8 == 0) && (act == MIVIT_ACT_NONE || lds % 8 == 0)) {
        prof_set_tag(MIVIT_PROF_LINEAR_DGRAD);
        return so->rowstream(true, dy, lddy, W, K, M, K, N, nullptr, MIVIT_ACT_NONE, act != MIVIT_ACT_NONE ? saved : nullptr,
                                lds, act, dres, lddr, dx, lddx, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, s);
    }
    if (dtype == MIVIT_BF16 && !dx_f32 && gemm_dma_supported(M, K, N, true) && lddy % 8 == 0 && lddx % 8 == 0 &&
        (!dres || lddr % 8 == 0) && (act == MIVIT_ACT_NONE || lds % 8 == 0) &&
        ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(dx) |
          reinterpret_cast<uintptr_t>(dres) | reinterpret_cast<uintptr_t>(act != MIVIT_ACT_NONE ? saved : nullptr)) & 15) == 0) {
        prof_set_tag(MIVIT_PROF_LINEAR_DGRAD);
        return launch_gemm_dma_dgrad(dy, lddy, W, M, N, K, act, saved, lds, dres, lddr, dx, lddx, s);
    }
    LinearDgradArgs a = {};
    a.dtype = dtype; a.dy = dy; a.dy_is_f32 = dtype == MIVIT_F32; a.lddy = lddy; a.W = W;
    a.w_is_bf16 = dtype != MIVIT_F32; a.M = M; a.N = N; a.K = K;
    a.act = act; a.saved = saved; a.lds = lds; a.dres = dres; a.lddr = lddr; a.dx = dx; a.lddx = lddx; a.dx_is_f32 = dx_f32;
    prof_set_tag(MIVIT_PROF_LINEAR_DGRAD);
    return launch_linear_dgrad(a, s);
}
int lin_wgrad(int dtype, const void *dy, int64_t lddy, const void *x, int x_f32, int64_t ldx, int M, int N, int K,
              float *dW, float *db, void *ws, size_t wsb, hipStream_t s) {
    const StreamOps *so = stream_ops(dtype);
    if (so && !x_f32 && dW && so->wgrad_dma_ok(M, N, K, lddy, ldx, dy, x) &&
        wsb >= so->wgrad_dma_ws(M, N, K) + linear_wgrad_ws_bytes(M, N, K)) {
        prof_set_tag(MIVIT_PROF_LINEAR_WGRAD);
        return so->wgrad_dma(dy, lddy, x, ldx, M, N, K, dW, db, ws, wsb, s);      // db (optional) from the same pass
    }
    if (so && !x_f32 && dW && so->wgrad_small_ok(M, N, K, lddy, ldx, dy, x) &&
        wsb >= so->wgrad_small_ws(M, N, K) && wsb >= linear_wgrad_ws_bytes(M, N, K)) {
        prof_set_tag(MIVIT_PROF_LINEAR_WGRAD);
        return so->wgrad_small(dy, lddy, x, ldx, M, N, K, dW, db, ws, wsb, s);      // db (optional) from the same pass
    }
    if (so && x_f32 && dW && ldx == K && so->embed_small_wgrad_ok(M, N, K, lddy, dy, x) && wsb >= so->embed_small_wgrad_ws(M, N, K)) {
        prof_set_tag(MIVIT_PROF_EMBED_WGRAD);
        return so->embed_small_wgrad(dy, lddy, static_cast<const float *>(x), M, N, K, dW, db, ws, wsb, s);
    }
    LinearWgradArgs a = {};
    a.dtype = dtype; a.dy = dy; a.dy_is_f32 = dtype == MIVIT_F32; a.lddy = lddy; a.x = x;
    a.x_is_f32 = x_f32 || dtype == MIVIT_F32; a.ldx = ldx; a.M = M; a.N = N; a.K = K; a.dW = dW; a.db = db;
    a.ws = ws; a.ws_bytes = wsb;
    prof_set_tag(x_f32 && K > 1024 ? MIVIT_PROF_EMBED_WGRAD : MIVIT_PROF_LINEAR_WGRAD);
    return launch_linear_wgrad(a, s);
}

// z = x W^T + b + resid;  y = LayerNorm(z)  (post-norm sub-layer, models.py:100-106): one row-stream launch when the
// block owns whole rows, otherwise GEMM + LayerNorm kernel.
int lin_res_ln(int dtype, const void *x, int64_t ldx, const void *W, const float *b, int M, int N, int K, const void *resid,
               void *z, const float *gamma, const float *beta, void *y, float *mean, float *rstd, hipStream_t s) {
    const StreamOps *so = stream_ops(dtype);
    if ((N == 128 || N == 64) && stream_gemm_supported(so, M, N, K, false, ldx, K, x, W)) {
        prof_set_tag(MIVIT_PROF_LINEAR_FWD);
        return so->rowstream(false, x, ldx, W, K, M, N, K, b, MIVIT_ACT_NONE, nullptr, 0, 0, resid, N, z, N, nullptr, gamma,
                                beta, y, N, mean, rstd, s);
    }
    RC(lin_fwd(dtype, x, 0, ldx, W, b, M, N, K, MIVIT_ACT_NONE, resid, N, z, N, nullptr, 0, s));
    LayerNormFwdArgs n = {};
    n.dtype = dtype; n.z = z; n.ldz = N; n.gamma = gamma; n.beta = beta; n.M = M; n.E = N; n.y = y; n.ldy = N;
    n.mean = mean; n.rstd = rstd;
    prof_set_tag(MIVIT_PROF_LN_FWD);
    return launch_layernorm_fwd(n, s);
}

// LayerNorm backward that also produces the bias gradient of the Linear feeding it (column sums of dz).
// *need_colsum is set when the scalar LayerNorm path ran and the caller must compute that bias gradient itself.
int ln_bwd_bias(LayerNormBwdArgs &a, float *db, bool *need_colsum, hipStream_t s) {
    a.dzsum = db;
    prof_set_tag(MIVIT_PROF_LN_BWD);
    const int rc = launch_layernorm_bwd(a, s);
    *need_colsum = (rc == 2);
    return rc == 2 ? 0 : rc;
}

int check_call(const mivit_plan *plan, int B, int T, size_t ws_bytes, bool bwd, const char *who) {
    MIVIT_CHECK(plan, "%s: null plan", who);
    MIVIT_CHECK(B > 0 && T > 0, "%s: empty batch (B=%d, T=%d)", who, B, T);
    const int S = T + (plan->c.use_regression_token ? 1 : 0);
    MIVIT_CHECK(!plan->c.use_pos_encoding || S <= MAX_TOKENS, "%s: %d tokens exceed the %d-entry positional table",
                who, S, MAX_TOKENS);
    const int Dh = plan->c.embed_dim / plan->c.num_heads;
    MIVIT_CHECK(S <= attention_max_seq(plan->c.dtype, Dh),
                "%s: sequence of %d tokens (head dim %d) does not fit the LDS-resident attention kernel (max %d)", who, S,
                Dh, attention_max_seq(plan->c.dtype, Dh));
    MIVIT_CHECK((int64_t)B * S * 3 * plan->c.embed_dim < (1ll << 31) && (int64_t)B * S * plan->c.hidden_dim < (1ll << 31),
                "%s: batch too large for 32-bit row indexing", who);
    const Ws w = make_ws(plan, B, T, bwd);
    MIVIT_CHECK(ws_bytes >= w.total, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, w.total);
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------
extern "C" mivit_plan *mivit_plan_create(const mivit_config *cfg) {
    if (!cfg) { mivit_set_error("plan_create: null config"); return nullptr; }
    const mivit_config &c = *cfg;
#define PLAN_CHECK(cond, ...) do { if (!(cond)) { mivit_set_error(__VA_ARGS__); return nullptr; } } while (0)
    PLAN_CHECK(c.abi_version == MIVIT_ABI_VERSION, "plan_create: ABI version %d != %d", c.abi_version, MIVIT_ABI_VERSION);
    PLAN_CHECK(c.dtype == MIVIT_F32 || c.dtype == MIVIT_BF16 || c.dtype == MIVIT_F16, "plan_create: bad dtype %d", c.dtype);
    PLAN_CHECK(c.embedding >= MIVIT_EMBED_LINEAR && c.embedding <= MIVIT_EMBED_EXTERNAL, "plan_create: bad embedding %d", c.embedding);
    PLAN_CHECK(c.embed_dim > 0 && c.num_heads > 0 && c.hidden_dim > 0 && c.num_layers >= 0, "plan_create: bad model dims");
    PLAN_CHECK(c.embed_dim % c.num_heads == 0, "embed_dim must be divisible by num_heads");
    PLAN_CHECK(c.embed_dim <= 1024, "plan_create: embed_dim %d > 1024 is not supported", c.embed_dim);
    PLAN_CHECK(c.embedding == MIVIT_EMBED_EXTERNAL || c.patch_size > 0, "plan_create: bad patch_size");
    PLAN_CHECK(c.activation >= MIVIT_ACT_RELU && c.activation <= MIVIT_ACT_GELU, "plan_create: unsupported activation %d", c.activation);
    PLAN_CHECK(c.fusion >= MIVIT_FUSION_NONE && c.fusion <= MIVIT_FUSION_LATE, "plan_create: bad fusion %d", c.fusion);
    PLAN_CHECK(c.fusion == MIVIT_FUSION_NONE || c.global_feature_dim > 0, "Must provide global_feature_dim if using global features");
    PLAN_CHECK(c.fusion != MIVIT_FUSION_EARLY || c.use_regression_token, "plan_create: early fusion needs the regression token");
    PLAN_CHECK(c.head_hidden > 0 && c.output_dim > 0, "plan_create: bad head dims");
#undef PLAN_CHECK
    mivit_plan *p = new mivit_plan();
    static std::atomic<uint64_t> next_uid{1};
    p->uid = next_uid.fetch_add(1);
    p->c = c;
    p->arena = 0;
    const int E = c.embed_dim, F = c.hidden_dim;
    p->head_in = c.fusion == MIVIT_FUSION_LATE ? 2 * E : E;
    // stage 0: final norm + (late-fusion feature projector) + head
    int64_t b0 = p->arena;
    p->tn_w = add_param(p, "transformer.norm.weight", E);
    p->tn_b = add_param(p, "transformer.norm.bias", E);
    if (c.fusion == MIVIT_FUSION_LATE) add_feature_projector(p);
    p->h0_w = add_param(p, "mlp_head.mlp.0.weight", (int64_t)c.head_hidden * p->head_in);
    p->h0_b = add_param(p, "mlp_head.mlp.0.bias", c.head_hidden);
    p->h3_w = add_param(p, "mlp_head.mlp.3.weight", (int64_t)c.output_dim * c.head_hidden);
    p->h3_b = add_param(p, "mlp_head.mlp.3.bias", c.output_dim);
    p->arena = (p->arena + 7) / 8 * 8;
    p->stages.push_back({b0, p->arena});
    // stages 1..L: encoder layers L-1 .. 0 (q/k/v weights and biases contiguous: one [3E,E] GEMM operand)
    p->layers.resize(c.num_layers);
    for (int l = c.num_layers - 1; l >= 0; --l) {
        b0 = p->arena;
        const std::string pre = "transformer.encoder_layers." + std::to_string(l) + ".";
        LayerParams &lp = p->layers[l];
        lp.qkv_w = add_param(p, pre + "self_attn.q_proj.weight", (int64_t)E * E);
        add_param(p, pre + "self_attn.k_proj.weight", (int64_t)E * E, false);
        add_param(p, pre + "self_attn.v_proj.weight", (int64_t)E * E, false);
        lp.qkv_b = add_param(p, pre + "self_attn.q_proj.bias", E);
        add_param(p, pre + "self_attn.k_proj.bias", E, false);
        add_param(p, pre + "self_attn.v_proj.bias", E, false);
        lp.out_w = add_param(p, pre + "self_attn.out_proj.weight", (int64_t)E * E);
        lp.out_b = add_param(p, pre + "self_attn.out_proj.bias", E);
        lp.n1_w = add_param(p, pre + "norm1.weight", E);
        lp.n1_b = add_param(p, pre + "norm1.bias", E);
        lp.fc1_w = add_param(p, pre + "feed_forward.fc1.weight", (int64_t)F * E);
        lp.fc1_b = add_param(p, pre + "feed_forward.fc1.bias", F);
        lp.fc2_w = add_param(p, pre + "feed_forward.fc2.weight", (int64_t)E * F);
        lp.fc2_b = add_param(p, pre + "feed_forward.fc2.bias", E);
        lp.n2_w = add_param(p, pre + "norm2.weight", E);
        lp.n2_b = add_param(p, pre + "norm2.bias", E);
        p->arena = (p->arena + 7) / 8 * 8;
        p->stages.push_back({b0, p->arena});
    }
    // last stage: token assembly + embedding (+ early-fusion feature projector)
    b0 = p->arena;
    p->reg = c.use_regression_token ? add_param(p, "reg_token", E) : -1;
    p->pos = c.use_pos_encoding ? add_param(p, "transformer.pos_embedding", (int64_t)MAX_TOKENS * E) : -1;
    p->n0_w = add_param(p, "norm.weight", E);
    p->n0_b = add_param(p, "norm.bias", E);
    if (c.fusion == MIVIT_FUSION_EARLY) add_feature_projector(p);
    p->emb_w = p->emb_b = -1;
    if (c.embedding == MIVIT_EMBED_LINEAR) {
        p->emb_w = add_param(p, "embedding.proj.weight", (int64_t)E * c.patch_size * c.patch_size);
        p->emb_b = add_param(p, "embedding.proj.bias", E);
    } else if (c.embedding == MIVIT_EMBED_CNN) {
        p->emb_w = add_param(p, "embedding.conv.weight", (int64_t)E * c.patch_size * c.patch_size);
        p->emb_b = add_param(p, "embedding.conv.bias", E);
    }
    p->arena = (p->arena + 7) / 8 * 8;
    p->stages.push_back({b0, p->arena});
    // q/k/v must be contiguous (E*E and E are multiples of 4 whenever E is): verify
    if ((int64_t)E * E % 4 != 0 || E % 4 != 0) {
        mivit_set_error("plan_create: embed_dim must be a multiple of 4 (got %d)", E);
        delete p;
        return nullptr;
    }
    return p;
}

extern "C" void mivit_plan_destroy(mivit_plan *plan) { delete plan; }
extern "C" int mivit_plan_num_params(const mivit_plan *plan) { return plan ? (int)plan->params.size() : 0; }
extern "C" const char *mivit_plan_param_name(const mivit_plan *plan, int i) {
    return (plan && i >= 0 && i < (int)plan->params.size()) ? plan->params[i].name.c_str() : nullptr;
}
extern "C" int64_t mivit_plan_param_offset(const mivit_plan *plan, int i) {
    return (plan && i >= 0 && i < (int)plan->params.size()) ? plan->params[i].offset : -1;
}
extern "C" int64_t mivit_plan_param_numel(const mivit_plan *plan, int i) {
    return (plan && i >= 0 && i < (int)plan->params.size()) ? plan->params[i].numel : -1;
}
extern "C" int64_t mivit_plan_arena_numel(const mivit_plan *plan) { return plan ? plan->arena : 0; }
extern "C" int mivit_plan_num_stages(const mivit_plan *plan) { return plan ? (int)plan->stages.size() : 0; }
extern "C" int mivit_plan_stage_range(const mivit_plan *plan, int stage, int64_t *begin, int64_t *end) {
    MIVIT_CHECK(plan && stage >= 0 && stage < (int)plan->stages.size(), "stage_range: bad stage %d", stage);
    if (begin) *begin = plan->stages[stage].first;
    if (end) *end = plan->stages[stage].second;
    return 0;
}
extern "C" size_t mivit_plan_workspace_bytes(const mivit_plan *plan, int B, int T, int need_backward) {
    if (!plan || B <= 0 || T <= 0) return 0;
    return make_ws(plan, B, T, need_backward != 0).total;
}

namespace {

// One forward / backward call, built once after check_call: the plan, the sizes derived from it and the caller's buffers.
struct Call {
    const mivit_plan *plan; const mivit_config &cfg;
    const int dt, E, F, H, Dh, L, B, T, off, S, M, Mt, f32;      // off: token row of a sequence's first frame; M / Mt: token / frame rows
    const bool bwd;               // the workspace is laid out for (and the forward keeps what) a backward needs
    const bool fused;             // the encoder layers run as fused blocks (fused_fwd.hip / fused_bwd.hip) ...
    const FusedOps *fo;           // ... of this table (null: per-operator layers)
    const bool rows;              // ... and the last layer's row-wise blocks on the B regression-token rows only (mode 2)
    const bool rows_exact;        // ... or only what leaves every sum as it was (mode 1)
    const int rq;                 // ... with these parts of the readout query (rq_parts; 0 in mode 3)
    const Ws w;
    void *ws; const float *P; float *G; hipStream_t s;      // workspace base, parameter arena, gradient arena (null in a forward)
    Call(const mivit_plan *p, int B_, int T_, bool bwd_, void *workspace, const float *params, float *grads, void *stream)
        : plan(p), cfg(p->c), dt(cfg.dtype), E(cfg.embed_dim), F(cfg.hidden_dim), H(cfg.num_heads), Dh(E / H), L(cfg.num_layers),
          B(B_), T(T_), off(cfg.use_regression_token ? 1 : 0), S(T + off), M(B * S), Mt(B * T), f32(dt == MIVIT_F32), bwd(bwd_),
          fused(L > 0 && fused_ok(dt, E, F, H, S)), fo(fused ? fused_ops(dt, E) : nullptr),
          rows(fused && cfg.use_regression_token && S > 1 && g_readout_rows == 2),
          rows_exact(fused && cfg.use_regression_token && S > 1 && g_readout_rows != 0 && g_readout_rows != 2),
          rq(rows_exact && g_readout_rows != 3 && attention_bwd_rows_ok(dt, S, Dh) ? rq_parts() : 0), w(make_ws(p, B, T, bwd)),
          ws(workspace), P(params), G(grads), s(static_cast<hipStream_t>(stream)) {}
    void *buf(size_t o) const { return at(ws, o); }                                   // workspace region at a Ws offset
    float *fbuf(size_t o) const { return static_cast<float *>(at(ws, o)); }
    const float *p(int64_t o) const { return P + o; }                                 // fp32 parameter (bias, LayerNorm affine, table)
    float *g(int64_t o) const { return G + o; }                                       // its gradient
    // GEMM weight operand: the 16-bit shadow of the arena (refreshed by every forward) in the 16-bit modes, the arena in fp32
    const void *W(int64_t o) const { return f32 ? (const void *)(P + o) : (const void *)(static_cast<const bf16 *>(buf(w.wsh)) + o); }
    const void *trunk_out() const { return L == 0 ? buf(w.x0) : (fused ? buf(w.xL) : buf(w.layer[L - 1].x2)); }      // = input of the final norm
};

// ---- forward ----------------------------------------------------------------------------------
// 1. frame embedding: one token per whole frame (models.py:146-199), [B*T, P*P] x [E, P*P]^T
int embed_fwd(const Call &c, const float *x) {
    const mivit_plan *p = c.plan;
    if (c.cfg.embedding == MIVIT_EMBED_EXTERNAL) return launch_convert(1, x, c.E, c.f32, c.buf(c.w.emb), c.E, c.Mt, c.E, 0, c.s, c.dt);
    const int K = c.cfg.patch_size * c.cfg.patch_size; const StreamOps *so = stream_ops(c.dt);
    if (so && so->embed_ok(c.dt, c.Mt, K, c.E)) {
        prof_set_tag(MIVIT_PROF_EMBED_FWD);
        return so->embed_fwd(x, c.W(p->emb_w), c.p(p->emb_b), c.buf(c.w.emb), c.Mt, K, c.E, c.s);
    }
    return lin_fwd(c.dt, x, 1, K, c.W(p->emb_w), c.p(p->emb_b), c.Mt, c.E, K, MIVIT_ACT_NONE, nullptr, 0, c.buf(c.w.emb), c.E, nullptr, 0, c.s);
}

// 2. token assembly: LayerNorm of the tokens, written behind the regression-token row, + positional table (models.py:334,347,138);
//    feature projector (models.py:316-320): Linear(Fg,E) -> ReLU -> Linear(E,E); regression token row (models.py:339-347)
int tokens_fwd(const Call &c, const float *features) {
    const mivit_plan *p = c.plan; const mivit_config &cfg = c.cfg; const Ws &w = c.w;
    const int dt = c.dt, E = c.E, B = c.B;
    LayerNormFwdArgs a = {};
    a.dtype = dt; a.z = c.buf(w.emb); a.ldz = E; a.gamma = c.p(p->n0_w); a.beta = c.p(p->n0_b); a.M = c.Mt; a.E = E;
    a.y = c.buf(w.x0); a.ldy = E; a.rows_per_seq = c.T; a.out_seq_stride = c.S; a.out_row_off = c.off;
    a.pos = cfg.use_pos_encoding ? c.p(p->pos) : nullptr; a.mean = c.fbuf(w.mean0); a.rstd = c.fbuf(w.rstd0);
    prof_set_tag(MIVIT_PROF_LN_FWD); RC(launch_layernorm_fwd(a, c.s));
    if (cfg.fusion != MIVIT_FUSION_NONE) {
        const int Fg = cfg.global_feature_dim;
        RC(lin_fwd(dt, features, 1, Fg, c.W(p->fp0_w), c.p(p->fp0_b), B, E, Fg, MIVIT_ACT_RELU, nullptr, 0, c.buf(w.fp_h), E, nullptr, 0, c.s));
        RC(lin_fwd(dt, c.buf(w.fp_h), 0, E, c.W(p->fp2_w), c.p(p->fp2_b), B, E, E, MIVIT_ACT_NONE, nullptr, 0, c.buf(w.fp_out), E, nullptr, 0, c.s));
    }
    if (cfg.use_regression_token)
        RC(launch_reg_token_fill(dt, c.buf(w.x0), B, c.S, E, c.p(p->reg), cfg.fusion == MIVIT_FUSION_EARLY ? c.buf(w.fp_out) : nullptr, a.pos, c.s));
    return 0;
}

// 3a. encoder layers as fused blocks (fused_fwd.hip): the layers hand each other NORMALISED tokens, the consumer applies the
//     producing LayerNorm's affine (folded into its weights); training keeps q|k|v for the backward kernels (h is recomputed
//     there), inference nothing; only the last block materialises x for the final norm
int layers_fwd_fused(const Call &c) {
    const float *gin = nullptr, *bin = nullptr;
    const void *nin = c.buf(c.w.x0);
    for (int l = 0; l < c.L; ++l) {
        const LayerParams &lp = c.plan->layers[l]; const Ws::L &b = c.w.layer[l];
        prof_set_tag(MIVIT_PROF_ATTN_BLOCK_FWD);
        RC(c.fo->attn_fwd(nin, gin, bin, c.W(lp.qkv_w), c.p(lp.qkv_b), c.W(lp.out_w), c.p(lp.out_b), c.p(lp.n1_w), c.p(lp.n1_b), c.B, c.S,
                          c.buf(b.ctx), c.buf(b.z1), c.fbuf(b.rstd1), nullptr, nullptr, nullptr, c.bwd ? c.buf(b.qkv) : nullptr,
                          (c.rq & 1) && l + 1 == c.L, c.s));
        if (c.rows_exact && l + 1 == c.L) {
            // mode 1: the same B-row launch; its outputs go to rows b * S of the full regions, where the final norm and the
            // unchanged backward look for them.  The backward reads every row of z2 / rstd2: the rows nobody computed are
            // zeroed (their d(x2) is 0, so any finite value gives the exact zeros the computed rows gave)
            const Ws &w = c.w; const size_t ts = dtype_size(c.dt); const int64_t SE = (int64_t)c.S * c.E;
            RC(launch_convert(0, c.buf(b.z1), SE, 0, c.buf(w.z1c), c.E, c.B, c.E, 0, c.s, c.dt));
            prof_set_tag(MIVIT_PROF_MLP_BLOCK_FWD);
            RC(c.fo->mlp_fwd(c.buf(w.z1c), c.p(lp.n1_w), c.p(lp.n1_b), c.W(lp.fc1_w), c.p(lp.fc1_b), c.W(lp.fc2_w), c.p(lp.fc2_b),
                             c.p(lp.n2_w), c.p(lp.n2_b), c.B, c.cfg.activation, c.buf(w.z2c), c.fbuf(w.rstd2c), c.buf(w.xLc), nullptr,
                             nullptr, nullptr, nullptr, c.s));
            RC(launch_convert(0, c.buf(w.xLc), c.E, 0, c.buf(w.xL), SE, c.B, c.E, 0, c.s, c.dt));
            if (c.bwd) {
                RC(launch_fill_zero(c.buf(b.z2), (size_t)c.M * c.E * ts, c.s));
                RC(launch_fill_zero(c.buf(b.rstd2), (size_t)c.M * 4, c.s));
                RC(launch_convert(0, c.buf(w.z2c), c.E, 0, c.buf(b.z2), SE, c.B, c.E, 0, c.s, c.dt));
                RC(launch_convert(1, c.fbuf(w.rstd2c), 1, 1, c.fbuf(b.rstd2), c.S, c.B, 1, 0, c.s, c.dt));
            }
            return 0;
        }
        if (c.rows && l + 1 == c.L) {
            // the head reads the regression-token row only: the feed-forward block of the last layer runs on those B rows, its
            // z2 / rstd2 / xL compact at the start of the full regions (the attention block above needs every row: K and V)
            RC(launch_convert(0, c.buf(b.z1), (int64_t)c.S * c.E, 0, c.buf(c.w.z1c), c.E, c.B, c.E, 0, c.s, c.dt));
            prof_set_tag(MIVIT_PROF_MLP_BLOCK_FWD);
            return c.fo->mlp_fwd(c.buf(c.w.z1c), c.p(lp.n1_w), c.p(lp.n1_b), c.W(lp.fc1_w), c.p(lp.fc1_b), c.W(lp.fc2_w), c.p(lp.fc2_b),
                                 c.p(lp.n2_w), c.p(lp.n2_b), c.B, c.cfg.activation, c.buf(b.z2), c.fbuf(b.rstd2), c.buf(c.w.xL), nullptr,
                                 nullptr, nullptr, nullptr, c.s);
        }
        prof_set_tag(MIVIT_PROF_MLP_BLOCK_FWD);
        RC(c.fo->mlp_fwd(c.buf(b.z1), c.p(lp.n1_w), c.p(lp.n1_b), c.W(lp.fc1_w), c.p(lp.fc1_b), c.W(lp.fc2_w), c.p(lp.fc2_b), c.p(lp.n2_w),
                         c.p(lp.n2_b), c.M, c.cfg.activation, c.buf(b.z2), c.fbuf(b.rstd2), l + 1 == c.L ? c.buf(c.w.xL) : nullptr,
                         nullptr, nullptr, nullptr, nullptr, c.s));
        nin = c.buf(b.z2); gin = c.p(lp.n2_w); bin = c.p(lp.n2_b);
    }
    return 0;
}

// 3b. encoder layers operator by operator (post-norm, models.py:97-108)
int layers_fwd_general(const Call &c) {
    const int dt = c.dt, E = c.E, F = c.F, M = c.M, act = c.cfg.activation;
    const void *xin = c.buf(c.w.x0);
    for (int l = 0; l < c.L; ++l) {
        const LayerParams &lp = c.plan->layers[l]; const Ws::L &b = c.w.layer[l];
        RC(lin_fwd(dt, xin, 0, E, c.W(lp.qkv_w), c.p(lp.qkv_b), M, 3 * E, E, MIVIT_ACT_NONE, nullptr, 0, c.buf(b.qkv), 3 * E, nullptr, 0, c.s));
        prof_set_tag(MIVIT_PROF_ATTN_FWD); RC(launch_attention_fwd(dt, c.buf(b.qkv), c.B, c.S, c.H, c.Dh, c.buf(b.ctx), c.s));
        RC(lin_res_ln(dt, c.buf(b.ctx), E, c.W(lp.out_w), c.p(lp.out_b), M, E, E, xin, c.buf(b.z1), c.p(lp.n1_w), c.p(lp.n1_b),
                      c.buf(b.x1), c.fbuf(b.mean1), c.fbuf(b.rstd1), c.s));
        RC(lin_fwd(dt, c.buf(b.x1), 0, E, c.W(lp.fc1_w), c.p(lp.fc1_b), M, F, E, act, nullptr, 0, c.buf(b.h), F,
                   act == MIVIT_ACT_GELU ? c.buf(b.u) : nullptr, 0, c.s));
        RC(lin_res_ln(dt, c.buf(b.h), F, c.W(lp.fc2_w), c.p(lp.fc2_b), M, E, F, c.buf(b.x1), c.buf(b.z2), c.p(lp.n2_w), c.p(lp.n2_b),
                      c.buf(b.x2), c.fbuf(b.mean2), c.fbuf(b.rstd2), c.s));
        xin = c.buf(b.x2);
    }
    return 0;
}

// 4. final LayerNorm + readout (models.py:141, :351-354).  Only the regression-token row is normalised when it is the
//    readout: the other rows of the final norm never reach the head.
int readout_fwd(const Call &c) {
    const Ws &w = c.w; LayerNormFwdArgs a = {};
    a.dtype = c.dt; a.z = c.trunk_out(); a.ldz = c.E; a.gamma = c.p(c.plan->tn_w); a.beta = c.p(c.plan->tn_b); a.E = c.E; a.ldy = c.E;
    a.mean = c.fbuf(w.meanF); a.rstd = c.fbuf(w.rstdF);
    prof_set_tag(MIVIT_PROF_LN_FWD);
    if (c.cfg.use_regression_token) {
        a.M = c.B; a.y = c.buf(w.pooled);
        if (!c.rows) { a.in_rows = 1; a.in_stride = c.S; a.in_off = 0; }          // (readout rows: the trunk's output is compact)
        return launch_layernorm_fwd(a, c.s);
    }
    a.M = c.M; a.y = c.buf(w.xF); RC(launch_layernorm_fwd(a, c.s));
    return launch_mean_pool_fwd(c.dt, c.buf(w.xF), c.B, c.S, c.E, c.buf(w.pooled), c.s);
}

// 5. late fusion concat (models.py:356-359) and the MLP head (models.py:268-276)
int head_fwd(const Call &c, float *out) {
    const mivit_plan *p = c.plan; const Ws &w = c.w;
    const int dt = c.dt, E = c.E, B = c.B, Hh = c.cfg.head_hidden, Hin = p->head_in, O = c.cfg.output_dim;
    const void *head_in = c.buf(w.pooled);
    if (c.cfg.fusion == MIVIT_FUSION_LATE) {
        RC(launch_convert(c.f32, c.buf(w.pooled), E, c.f32, c.buf(w.head_in), 2 * E, B, E, 0, c.s, dt));
        RC(launch_convert(c.f32, c.buf(w.fp_out), E, c.f32, col_ptr(c.buf(w.head_in), E, dt), 2 * E, B, E, 0, c.s, dt));
        head_in = c.buf(w.head_in);
    }
    RC(lin_fwd(dt, head_in, 0, Hin, c.W(p->h0_w), c.p(p->h0_b), B, Hh, Hin, MIVIT_ACT_RELU, nullptr, 0, c.buf(w.hh), Hh, nullptr, 0, c.s));
    return lin_fwd(dt, c.buf(w.hh), 0, Hh, c.W(p->h3_w), c.p(p->h3_b), B, O, Hh, MIVIT_ACT_NONE, nullptr, 0, out, O, nullptr, 1, c.s);
}

int forward_impl(const mivit_plan *plan, const float *params, const float *x, const float *features, int B, int T,
                        void *workspace, size_t workspace_bytes, int need_backward, float *out, void *stream) {
    RC(check_call(plan, B, T, workspace_bytes, need_backward != 0, "mivit_forward"));
    MIVIT_CHECK(params && x && workspace && out, "mivit_forward: null pointer");
    MIVIT_CHECK(plan->c.fusion == MIVIT_FUSION_NONE || features, "Global features required for %s fusion",
                plan->c.fusion == MIVIT_FUSION_EARLY ? "early" : "late");
    const Call c(plan, B, T, need_backward != 0, workspace, params, nullptr, stream);
    // 16-bit modes: one conversion of the whole fp32 arena per step; every GEMM then stages 16-bit weights
    if (!c.f32) RC(launch_convert(1, c.P, plan->arena, 0, c.buf(c.w.wsh), plan->arena, 1, (int)plan->arena, 0, c.s, c.dt));
    RC(embed_fwd(c, x));
    RC(tokens_fwd(c, features));
    RC(c.fused ? layers_fwd_fused(c) : layers_fwd_general(c));
    RC(readout_fwd(c));
    return head_fwd(c, out);
}

// ---- backward: one function per stage (mivit_plan::stages) and, for the encoder layers, per path.  dxa holds the gradient of
// ---- a stage's output on entry and of its input on exit ----------------------------------------
// backward of the feature projector given d(fp_out) (rows of `dy`, leading dim lddy)
int feature_projector_bwd(const Call &c, const float *features, const void *dy, int64_t lddy, float *dfeatures) {
    const mivit_plan *p = c.plan; const Ws &w = c.w;
    const int dt = c.dt, E = c.E, B = c.B, Fg = c.cfg.global_feature_dim;
    RC(lin_wgrad(dt, dy, lddy, c.buf(w.fp_h), 0, E, B, E, E, c.g(p->fp2_w), c.g(p->fp2_b), c.buf(w.wgrad), w.wgrad_bytes, c.s));
    RC(lin_dgrad(dt, dy, lddy, c.W(p->fp2_w), B, E, E, MIVIT_ACT_RELU, c.buf(w.fp_h), E, nullptr, 0, c.buf(w.d_fp_h), E, 0, c.s));
    RC(lin_wgrad(dt, c.buf(w.d_fp_h), E, features, 1, Fg, B, E, Fg, c.g(p->fp0_w), c.g(p->fp0_b), c.buf(w.wgrad), w.wgrad_bytes, c.s));
    if (dfeatures) RC(lin_dgrad(dt, c.buf(w.d_fp_h), E, c.W(p->fp0_w), B, E, Fg, MIVIT_ACT_NONE, nullptr, 0, nullptr, 0, dfeatures, Fg, 1, c.s));
    return 0;
}

// stage 0: head + (late fusion) feature projector + final norm
int head_bwd(const Call &c, const float *dout, const float *features, float *dfeatures) {
    const mivit_plan *p = c.plan; const Ws &w = c.w;
    const int dt = c.dt, E = c.E, B = c.B, Hh = c.cfg.head_hidden, Hin = p->head_in, O = c.cfg.output_dim;
    void *wg = c.buf(w.wgrad); const size_t wgb = w.wgrad_bytes;
    const void *head_in = c.cfg.fusion == MIVIT_FUSION_LATE ? c.buf(w.head_in) : c.buf(w.pooled), *dy = dout;
    if (!c.f32) { RC(launch_convert(1, dout, O, 0, c.buf(w.dout_t), O, B, O, 0, c.s, dt)); dy = c.buf(w.dout_t); }
    RC(lin_wgrad(dt, dy, O, c.buf(w.hh), 0, Hh, B, O, Hh, c.g(p->h3_w), c.g(p->h3_b), wg, wgb, c.s));
    RC(lin_dgrad(dt, dy, O, c.W(p->h3_w), B, O, Hh, MIVIT_ACT_RELU, c.buf(w.hh), Hh, nullptr, 0, c.buf(w.d_hh), Hh, 0, c.s));
    RC(lin_wgrad(dt, c.buf(w.d_hh), Hh, head_in, 0, Hin, B, Hh, Hin, c.g(p->h0_w), c.g(p->h0_b), wg, wgb, c.s));
    RC(lin_dgrad(dt, c.buf(w.d_hh), Hh, c.W(p->h0_w), B, Hh, Hin, MIVIT_ACT_NONE, nullptr, 0, nullptr, 0, c.buf(w.d_head_in), Hin, 0, c.s));
    if (c.cfg.fusion == MIVIT_FUSION_LATE) RC(feature_projector_bwd(c, features, col_ptr(c.buf(w.d_head_in), E, dt), Hin, dfeatures));
    LayerNormBwdArgs a = {};
    a.dtype = dt; a.z = c.trunk_out(); a.ldz = E; a.gamma = c.p(p->tn_w); a.mean = c.fbuf(w.meanF); a.rstd = c.fbuf(w.rstdF);
    a.E = E; a.dz = c.buf(w.dxa); a.lddz = E; a.dgamma = c.g(p->tn_w); a.dbeta = c.g(p->tn_b); a.ws = c.buf(w.ln); a.ws_bytes = w.ln_bytes;
    if (c.cfg.use_regression_token) {
        // d(trunk output) is non-zero in the regression-token rows only: [B,E] compact for the readout-row backward of the last
        // layer, otherwise those rows of a zeroed [M,E]
        a.dy = c.buf(w.d_head_in); a.lddy = Hin; a.M = B;
        if (!c.rows) {
            RC(launch_fill_zero(c.buf(w.dxa), (size_t)c.M * E * dtype_size(dt), c.s));
            a.z_rows = 1; a.z_stride = c.S; a.z_off = 0;
        }
    } else {
        const void *dp = c.buf(w.d_head_in);
        if (Hin != E) {
            RC(launch_convert(c.f32, c.buf(w.d_head_in), Hin, c.f32, c.buf(w.d_pool_c), E, B, E, 0, c.s, dt));
            dp = c.buf(w.d_pool_c);
        }
        RC(launch_mean_pool_bwd(dt, dp, B, c.S, E, c.buf(w.dxb), c.s));
        a.dy = c.buf(w.dxb); a.lddy = E; a.M = c.M;
    }
    prof_set_tag(MIVIT_PROF_LN_BWD);
    return launch_layernorm_bwd(a, c.s);
}

// The weight-gradient workspace as the fused backward blocks of one layer get it.  Deferred slab reductions (slab_defer.h) need
// the three blocks' slabs to coexist: one region each, back to back.  Otherwise every block has the whole workspace.
struct FusedBwdWs { bool defer; struct Region { void *ptr; size_t bytes; } mlp, attn_out, qkv; };
FusedBwdWs fused_bwd_ws(const Call &c, bool want_defer) {
    uint8_t *wg = static_cast<uint8_t *>(c.buf(c.w.wgrad));
    const size_t wgb = c.w.wgrad_bytes, n_mlp = c.fo->mlp_bwd_ws(c.M), n_ao = c.fo->attn_out_bwd_ws(c.M);
    if (!want_defer || wgb < n_mlp + n_ao + c.fo->qkv_bwd_ws(c.M)) return {false, {wg, wgb}, {wg, wgb}, {wg, wgb}};
    return {true, {wg, wgb}, {wg + n_mlp, wgb - n_mlp}, {wg + n_mlp + n_ao, wgb - n_mlp - n_ao}};
}

// stages 1..L, fused blocks (fused_bwd.hip): z1 / z2 hold xhat (no means), the Linear inputs x1 / x_in exist only as xhat of the
// producing norm: their weight gradients are taken against xhat and corrected by the affine fix-up.  Four launches + ONE slab reduction.
int layer_bwd_fused(const Call &c, int l) {
    static const bool qkv_split = getenv("MIVIT_NO_QKV_BWD") != nullptr;                        // A/B: the two launches qkv_bwd replaces
    static const bool no_defer = getenv("MIVIT_NO_SLAB_DEFER") != nullptr || qkv_split;         // A/B: one reduction behind every block
    const Ws &w = c.w; const Ws::L &b = w.layer[l]; const LayerParams &lp = c.plan->layers[l];
    const int dt = c.dt, E = c.E, M = c.M;
    // x_in of layers l > 0 is the normalised output of the layer below, to be read through that layer's LayerNorm-2 affine
    const void *xin = l > 0 ? c.buf(w.layer[l - 1].z2) : c.buf(w.x0);
    const float *gin = l > 0 ? c.p(c.plan->layers[l - 1].n2_w) : nullptr, *bin = l > 0 ? c.p(c.plan->layers[l - 1].n2_b) : nullptr;
    void *dx1 = c.buf(w.dxb), *dz1 = c.buf(w.dF);      // where d(x1) arrives / where LayerNorm-1's backward puts d(z1)
    const FusedBwdWs r = fused_bwd_ws(c, !no_defer);
    SlabDefer slabs(r.defer);
    // readout query (mode 1, last layer): d(x1), d(z1), d(ctx) and dq are exact zeros outside row 0 of every sequence -- the
    // kernels below neither read nor write those zeros
    const int rq = l + 1 == c.L ? c.rq : 0;
    prof_set_tag(MIVIT_PROF_MLP_BLOCK_BWD);          // feed-forward block: d(x2) -> d(x1), all six parameter gradients
    RC(c.fo->mlp_bwd(c.buf(w.dxa), c.buf(b.z2), c.fbuf(b.rstd2), c.p(lp.n2_w), c.buf(b.z1), c.p(lp.n1_w), c.p(lp.n1_b), c.W(lp.fc1_w),
                     c.p(lp.fc1_b), c.W(lp.fc2_w), M, c.cfg.activation, dx1, c.g(lp.fc1_w), c.g(lp.fc1_b), c.g(lp.fc2_w), c.g(lp.fc2_b),
                     c.g(lp.n2_w), c.g(lp.n2_b), r.mlp.ptr, r.mlp.bytes, c.s));
    prof_set_tag(MIVIT_PROF_ATTN_OUT_BWD);           // LayerNorm-1 backward + out-projection weight / data gradient
    RC(c.fo->attn_out_bwd(dx1, c.buf(b.z1), c.fbuf(b.rstd1), c.p(lp.n1_w), c.buf(b.ctx), c.W(lp.out_w), M, (rq & 2) ? c.S : 0, dz1,
                          c.buf(w.dctx), c.g(lp.out_w), c.g(lp.out_b), c.g(lp.n1_w), c.g(lp.n1_b), r.attn_out.ptr, r.attn_out.bytes, c.s));
    prof_set_tag(MIVIT_PROF_ATTN_CORE_BWD);
    if (c.rows_exact && l + 1 == c.L && attention_bwd_rows_ok(dt, c.S, c.Dh))       // d(ctx) is zero behind row 0 of every sequence
        RC(launch_attention_bwd_q_rows(dt, c.buf(b.qkv), c.buf(w.dctx), (int64_t)c.S * E, 1, (rq & 1) != 0, c.B, c.S,
                                       c.H, c.Dh, c.buf(w.dqkv), c.s));
    else
        RC(launch_attention_bwd(dt, c.buf(b.qkv), c.buf(w.dctx), c.B, c.S, c.H, c.Dh, c.buf(w.dqkv), c.s));
    if (!qkv_split) {
        // q|k|v projection: weight, bias and data gradient (+ the residual branch's d(z1)) in ONE pass over dqkv; the affine fix-up
        // of the weight gradient, dW diag(gamma) + db (x) beta, rides on the kernel's slab writes
        ProfPin pin(MIVIT_PROF_QKV_BWD);
        RC(c.fo->qkv_bwd(c.buf(w.dqkv), xin, c.W(lp.qkv_w), dz1, M, c.buf(w.dxa), c.g(lp.qkv_w), c.g(lp.qkv_b), gin, bin, r.qkv.ptr, r.qkv.bytes, c.s));
        return slabs.flush(c.s);
    }
    ProfPin pin(MIVIT_PROF_QKV_WGRAD);
    RC(lin_wgrad(dt, c.buf(w.dqkv), 3 * E, xin, 0, E, M, 3 * E, E, c.g(lp.qkv_w), c.g(lp.qkv_b), r.qkv.ptr, r.qkv.bytes, c.s));
    if (l > 0) RC(launch_affine_fixup(c.g(lp.qkv_w), c.g(lp.qkv_b), gin, bin, 3 * E, E, c.s));
    pin.set(MIVIT_PROF_QKV_DGRAD);
    return lin_dgrad(dt, c.buf(w.dqkv), 3 * E, c.W(lp.qkv_w), M, 3 * E, E, MIVIT_ACT_NONE, nullptr, 0, dz1, E, c.buf(w.dxa), E, 0, c.s);
}

// stage 1 under the readout-row pruning: d(x2) of the last layer arrives as the B regression-token rows (every other row is
// an exact zero, and with it d(z2), d(x1), d(z1) and d(ctx) of that row).  The same four kernels: the feed-forward block and
// LayerNorm-1 / out-projection on gathered [B, .] operands, the attention core told that one query row per sequence carries a
// gradient (d(k), d(v) are dense), the q|k|v projection on all rows with the compact d(z1) scattered into a zeroed residual.
int last_layer_bwd_rows(const Call &c) {
    static const bool qkv_split = getenv("MIVIT_NO_QKV_BWD") != nullptr;
    static const bool no_defer = getenv("MIVIT_NO_SLAB_DEFER") != nullptr || qkv_split;
    const int l = c.L - 1;
    const Ws &w = c.w; const Ws::L &b = w.layer[l]; const LayerParams &lp = c.plan->layers[l];
    const int dt = c.dt, E = c.E, M = c.M, B = c.B; const int64_t SE = (int64_t)c.S * E;
    const void *xin = l > 0 ? c.buf(w.layer[l - 1].z2) : c.buf(w.x0);
    const float *gin = l > 0 ? c.p(c.plan->layers[l - 1].n2_w) : nullptr, *bin = l > 0 ? c.p(c.plan->layers[l - 1].n2_b) : nullptr;
    void *dx1 = c.buf(w.dxb), *dz1 = c.buf(w.dF);          // compact d(x1) / full d(z1)
    const FusedBwdWs r = fused_bwd_ws(c, !no_defer);
    SlabDefer slabs(r.defer);
    RC(launch_convert(1, c.fbuf(b.rstd1), c.S, 1, c.fbuf(w.rstd1c), 1, B, 1, 0, c.s, dt));
    RC(launch_convert(0, c.buf(b.ctx), SE, 0, c.buf(w.ctxc), E, B, E, 0, c.s, dt));
    prof_set_tag(MIVIT_PROF_MLP_BLOCK_BWD);
    RC(c.fo->mlp_bwd(c.buf(w.dxa), c.buf(b.z2), c.fbuf(b.rstd2), c.p(lp.n2_w), c.buf(w.z1c), c.p(lp.n1_w), c.p(lp.n1_b), c.W(lp.fc1_w),
                     c.p(lp.fc1_b), c.W(lp.fc2_w), B, c.cfg.activation, dx1, c.g(lp.fc1_w), c.g(lp.fc1_b), c.g(lp.fc2_w), c.g(lp.fc2_b),
                     c.g(lp.n2_w), c.g(lp.n2_b), r.mlp.ptr, r.mlp.bytes, c.s));
    prof_set_tag(MIVIT_PROF_ATTN_OUT_BWD);
    RC(c.fo->attn_out_bwd(dx1, c.buf(w.z1c), c.fbuf(w.rstd1c), c.p(lp.n1_w), c.buf(w.ctxc), c.W(lp.out_w), B, 0, c.buf(w.dz1c), c.buf(w.dctxc),
                          c.g(lp.out_w), c.g(lp.out_b), c.g(lp.n1_w), c.g(lp.n1_b), r.attn_out.ptr, r.attn_out.bytes, c.s));
    if (attention_bwd_rows_ok(dt, c.S, c.Dh)) {
        prof_set_tag(MIVIT_PROF_ATTN_CORE_BWD);
        RC(launch_attention_bwd_q_rows(dt, c.buf(b.qkv), c.buf(w.dctxc), E, 1, false, B, c.S, c.H, c.Dh, c.buf(w.dqkv), c.s));
    } else {          // (MIVIT_ATTN_BWD=1: the first attention kernel reads every row of d(ctx))
        RC(launch_fill_zero(c.buf(w.dctx), (size_t)M * E * dtype_size(dt), c.s));
        RC(launch_convert(0, c.buf(w.dctxc), E, 0, c.buf(w.dctx), SE, B, E, 0, c.s, dt));
        prof_set_tag(MIVIT_PROF_ATTN_CORE_BWD);
        RC(launch_attention_bwd(dt, c.buf(b.qkv), c.buf(w.dctx), B, c.S, c.H, c.Dh, c.buf(w.dqkv), c.s));
    }
    RC(launch_fill_zero(dz1, (size_t)M * E * dtype_size(dt), c.s));
    RC(launch_convert(0, c.buf(w.dz1c), E, 0, dz1, SE, B, E, 0, c.s, dt));
    if (!qkv_split) {
        ProfPin pin(MIVIT_PROF_QKV_BWD);
        RC(c.fo->qkv_bwd(c.buf(w.dqkv), xin, c.W(lp.qkv_w), dz1, M, c.buf(w.dxa), c.g(lp.qkv_w), c.g(lp.qkv_b), gin, bin, r.qkv.ptr, r.qkv.bytes, c.s));
        return slabs.flush(c.s);
    }
    ProfPin pin(MIVIT_PROF_QKV_WGRAD);
    RC(lin_wgrad(dt, c.buf(w.dqkv), 3 * E, xin, 0, E, M, 3 * E, E, c.g(lp.qkv_w), c.g(lp.qkv_b), r.qkv.ptr, r.qkv.bytes, c.s));
    if (l > 0) RC(launch_affine_fixup(c.g(lp.qkv_w), c.g(lp.qkv_b), gin, bin, 3 * E, E, c.s));
    pin.set(MIVIT_PROF_QKV_DGRAD);
    return lin_dgrad(dt, c.buf(w.dqkv), 3 * E, c.W(lp.qkv_w), M, 3 * E, E, MIVIT_ACT_NONE, nullptr, 0, dz1, E, c.buf(w.dxa), E, 0, c.s);
}

// stages 1..L, operator by operator
int layer_bwd_general(const Call &c, int l) {
    const Ws &w = c.w; const Ws::L &b = w.layer[l]; const LayerParams &lp = c.plan->layers[l];
    const int dt = c.dt, E = c.E, F = c.F, M = c.M, act = c.cfg.activation;
    const void *xin = l > 0 ? c.buf(w.layer[l - 1].x2) : c.buf(w.x0);
    void *wg = c.buf(w.wgrad), *dxa = c.buf(w.dxa), *dxb = c.buf(w.dxb); const size_t wgb = w.wgrad_bytes;
    bool cs = false; LayerNormBwdArgs n2 = {};
    n2.dtype = dt; n2.dy = dxa; n2.lddy = E; n2.z = c.buf(b.z2); n2.ldz = E; n2.gamma = c.p(lp.n2_w); n2.mean = c.fbuf(b.mean2);
    n2.rstd = c.fbuf(b.rstd2); n2.M = M; n2.E = E; n2.dz = dxb; n2.lddz = E; n2.dgamma = c.g(lp.n2_w); n2.dbeta = c.g(lp.n2_b);
    n2.ws = c.buf(w.ln); n2.ws_bytes = w.ln_bytes;
    RC(ln_bwd_bias(n2, c.g(lp.fc2_b), &cs, c.s));                                             // dxb = d(z2), fc2.bias grad
    RC(lin_wgrad(dt, dxb, E, c.buf(b.h), 0, F, M, E, F, c.g(lp.fc2_w), cs ? c.g(lp.fc2_b) : nullptr, wg, wgb, c.s));
    RC(lin_dgrad(dt, dxb, E, c.W(lp.fc2_w), M, E, F, act, act == MIVIT_ACT_GELU ? c.buf(b.u) : c.buf(b.h), F, nullptr, 0, c.buf(w.dF), F, 0, c.s));
    RC(lin_wgrad(dt, c.buf(w.dF), F, c.buf(b.x1), 0, E, M, F, E, c.g(lp.fc1_w), c.g(lp.fc1_b), wg, wgb, c.s));
    RC(lin_dgrad(dt, c.buf(w.dF), F, c.W(lp.fc1_w), M, F, E, MIVIT_ACT_NONE, nullptr, 0, dxb, E, dxa, E, 0, c.s));      // dxa = d(x1)
    LayerNormBwdArgs n1 = n2;
    n1.dy = dxa; n1.z = c.buf(b.z1); n1.gamma = c.p(lp.n1_w); n1.mean = c.fbuf(b.mean1); n1.rstd = c.fbuf(b.rstd1);
    n1.dz = dxb; n1.dgamma = c.g(lp.n1_w); n1.dbeta = c.g(lp.n1_b);
    RC(ln_bwd_bias(n1, c.g(lp.out_b), &cs, c.s));                                             // dxb = d(z1), out_proj.bias grad
    RC(lin_wgrad(dt, dxb, E, c.buf(b.ctx), 0, E, M, E, E, c.g(lp.out_w), cs ? c.g(lp.out_b) : nullptr, wg, wgb, c.s));
    RC(lin_dgrad(dt, dxb, E, c.W(lp.out_w), M, E, E, MIVIT_ACT_NONE, nullptr, 0, nullptr, 0, c.buf(w.dctx), E, 0, c.s));
    prof_set_tag(MIVIT_PROF_ATTN_BWD);
    RC(launch_attention_bwd(dt, c.buf(b.qkv), c.buf(w.dctx), c.B, c.S, c.H, c.Dh, c.buf(w.dqkv), c.s));
    RC(lin_wgrad(dt, c.buf(w.dqkv), 3 * E, xin, 0, E, M, 3 * E, E, c.g(lp.qkv_w), c.g(lp.qkv_b), wg, wgb, c.s));
    return lin_dgrad(dt, c.buf(w.dqkv), 3 * E, c.W(lp.qkv_w), M, 3 * E, E, MIVIT_ACT_NONE, nullptr, 0, dxb, E, dxa, E, 0, c.s);      // dxa = d(x_in)
}

// last stage: token assembly + embedding; dxa holds d(x0) [B,S,E]
int embed_bwd(const Call &c, const float *x, const float *features, float *dfeatures, float *dx_tokens) {
    const mivit_plan *p = c.plan; const mivit_config &cfg = c.cfg; const Ws &w = c.w;
    const int dt = c.dt, E = c.E, B = c.B, S = c.S, Mt = c.Mt;
    void *wg = c.buf(w.wgrad); const size_t wgb = w.wgrad_bytes;
    if (cfg.use_pos_encoding) {
        RC(launch_fill_zero(c.g(p->pos), (size_t)MAX_TOKENS * E * sizeof(float), c.s));
        RC(launch_batch_colsum(dt, c.buf(w.dxa), B, S, E, 0, S, c.g(p->pos), c.buf(w.colsum), w.colsum_bytes, c.s));
    }
    if (cfg.use_regression_token) RC(launch_batch_colsum(dt, c.buf(w.dxa), B, S, E, 0, 1, c.g(p->reg), c.buf(w.colsum), w.colsum_bytes, c.s));
    if (cfg.fusion == MIVIT_FUSION_EARLY) RC(feature_projector_bwd(c, features, c.buf(w.dxa), (int64_t)S * E, dfeatures));
    LayerNormBwdArgs a = {};
    a.dtype = dt; a.dy = c.buf(w.dxa); a.lddy = E; a.z = c.buf(w.emb); a.ldz = E; a.gamma = c.p(p->n0_w); a.mean = c.fbuf(w.mean0);
    a.rstd = c.fbuf(w.rstd0); a.M = Mt; a.E = E; a.rows_per_seq = c.T; a.in_seq_stride = S; a.in_row_off = c.off;
    a.dz = c.buf(w.dxb); a.lddz = E; a.dgamma = c.g(p->n0_w); a.dbeta = c.g(p->n0_b); a.ws = c.buf(w.ln); a.ws_bytes = w.ln_bytes;
    if (cfg.embedding == MIVIT_EMBED_EXTERNAL) {
        prof_set_tag(MIVIT_PROF_LN_BWD); RC(launch_layernorm_bwd(a, c.s));                        // dxb = d(tokens)
        if (dx_tokens) RC(launch_convert(c.f32, c.buf(w.dxb), E, 1, dx_tokens, E, Mt, E, 0, c.s, dt));
        return 0;
    }
    bool cs = false;
    RC(ln_bwd_bias(a, c.g(p->emb_b), &cs, c.s));                                                  // dxb = d(embedding out)
    const int K = cfg.patch_size * cfg.patch_size; const StreamOps *so = stream_ops(dt);
    if (so && so->embed_ok(dt, Mt, K, E)) {
        prof_set_tag(MIVIT_PROF_EMBED_WGRAD);
        RC(so->embed_wgrad(c.buf(w.dxb), x, c.g(p->emb_w), Mt, K, E, wg, wgb, c.s));
        if (cs) RC(lin_wgrad(dt, c.buf(w.dxb), E, x, 1, K, Mt, E, K, nullptr, c.g(p->emb_b), wg, wgb, c.s));
        return 0;
    }
    return lin_wgrad(dt, c.buf(w.dxb), E, x, 1, K, Mt, E, K, c.g(p->emb_w), cs ? c.g(p->emb_b) : nullptr, wg, wgb, c.s);
}

int backward_impl(const mivit_plan *plan, const float *params, const float *x, const float *features, int B, int T,
                         void *workspace, size_t workspace_bytes, const float *dout, float *grads, float *dfeatures,
                         float *dx_tokens, int stage_begin, int stage_end, void *stream) {
    RC(check_call(plan, B, T, workspace_bytes, true, "mivit_backward"));
    MIVIT_CHECK(params && x && workspace && dout && grads, "mivit_backward: null pointer");
    MIVIT_CHECK(stage_begin >= 0 && stage_begin <= stage_end && stage_end <= (int)plan->stages.size(),
                "mivit_backward: bad stage range [%d,%d)", stage_begin, stage_end);
    MIVIT_CHECK(plan->c.fusion == MIVIT_FUSION_NONE || features, "mivit_backward: features required");
    const Call c(plan, B, T, true, workspace, params, grads, stream);
    for (int st = stage_begin; st < stage_end; ++st) {
        if (st == 0) RC(head_bwd(c, dout, features, dfeatures));
        else if (st == 1 && c.rows) RC(last_layer_bwd_rows(c));
        else if (st <= c.L) RC(c.fused ? layer_bwd_fused(c, c.L - st) : layer_bwd_general(c, c.L - st));      // layers L-1 .. 0
        else RC(embed_bwd(c, x, features, dfeatures, dx_tokens));
    }
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C-ABI entry points.  Small problems are launch-bound (~100 short kernels per call): a call whose arguments were seen
// before is captured once into a hipGraph on an internal stream and replayed on the caller's stream afterwards.
// ------------------------------------------------------------------------------------------------
// "Small" = launch-bound: the kernels of a narrow model are short at row counts where those of a wide one are not, so the
// limit is on activation ELEMENTS (token rows x embedding width; 65 536 rows at E = 128, 131 072 at the reference's E = 64:
// its Framerate shape at 4096 sequences per step, ~100 launches of 10-30 us each, is replayed instead of launched).
static bool graph_sized(const mivit_plan *plan, int B, int T) {
    return plan && (int64_t)B * (T + 1) * plan->c.embed_dim <= 65536LL * 128;
}

extern "C" int mivit_forward(const mivit_plan *plan, const float *params, const float *x, const float *features, int B, int T,
                             void *workspace, size_t workspace_bytes, int need_backward, float *out, void *stream) {
    const auto body = [&](hipStream_t cs) {
        return forward_impl(plan, params, x, features, B, T, workspace, workspace_bytes, need_backward, out, cs);
    };
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!graph_sized(plan, B, T)) return body(s);
    const uint64_t key[] = {1, plan->uid, (uint64_t)params, (uint64_t)x, (uint64_t)features, (uint64_t)B, (uint64_t)T,
                            (uint64_t)workspace, (uint64_t)workspace_bytes, (uint64_t)need_backward, (uint64_t)out,
                            (uint64_t)g_readout_rows};          // (the switch changes the launch sequence)
    return graph_run(key, (int)(sizeof(key) / sizeof(key[0])), s, body);
}

extern "C" int mivit_backward(const mivit_plan *plan, const float *params, const float *x, const float *features, int B,
                              int T, void *workspace, size_t workspace_bytes, const float *dout, float *grads,
                              float *dfeatures, float *dx_tokens, int stage_begin, int stage_end, void *stream) {
    const auto body = [&](hipStream_t cs) {
        return backward_impl(plan, params, x, features, B, T, workspace, workspace_bytes, dout, grads, dfeatures, dx_tokens,
                             stage_begin, stage_end, cs);
    };
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!graph_sized(plan, B, T)) return body(s);
    const uint64_t key[] = {2, plan->uid, (uint64_t)params, (uint64_t)x, (uint64_t)features, (uint64_t)B, (uint64_t)T,
                            (uint64_t)workspace, (uint64_t)workspace_bytes, (uint64_t)dout, (uint64_t)grads,
                            (uint64_t)dfeatures, (uint64_t)dx_tokens, (uint64_t)stage_begin, (uint64_t)stage_end,
                            (uint64_t)g_readout_rows};
    return graph_run(key, (int)(sizeof(key) / sizeof(key[0])), s, body);
}
