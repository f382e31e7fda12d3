/*
 * mivit_hip.h -- C-ABI of libmivit_hip.so: the MI355X (gfx950) implementation of the MiViT hot path.
 *
 * The reference (Biomedical-Imaging-Group/MolecularDiffusion_MiViT) has no FFI: its path is a tree of
 * torch.nn modules in helpers/models.py.  This header is the boundary a binding would target; every entry
 * point cites the reference lines whose arithmetic it replaces.  Conventions:
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer unless named host_*;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued, nothing syncs;
 *   - `dtype`: MIVIT_F32 (fp32 operands, v_mfma_f32_16x16x4_f32, the 1e-4 parity mode) or MIVIT_BF16
 *     (bf16 operands / stored activations, fp32 accumulate, fp32 LayerNorm+softmax statistics);
 *     master weights, biases, LayerNorm parameters and all weight gradients are ALWAYS fp32;
 *   - return value 0 = OK, non-zero = error; mivit_last_error() returns a thread-local message;
 *   - the library never allocates or frees device memory: callers pass workspaces
 *     (sizes from mivit_*_workspace_bytes / mivit_plan_workspace_bytes).
 */
#ifndef MIVIT_HIP_H
#define MIVIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIVIT_ABI_VERSION 1

enum { MIVIT_F32 = 0, MIVIT_BF16 = 1, MIVIT_F16 = 2, MIVIT_F64 = 3 };   /* F64: trajectory descriptors only */
enum { MIVIT_ACT_NONE = 0, MIVIT_ACT_RELU = 1, MIVIT_ACT_LEAKY_RELU = 2, MIVIT_ACT_GELU = 3 };
enum { MIVIT_EMBED_LINEAR = 0, MIVIT_EMBED_CNN = 1, MIVIT_EMBED_EXTERNAL = 2 };
enum { MIVIT_FUSION_NONE = 0, MIVIT_FUSION_EARLY = 1, MIVIT_FUSION_LATE = 2 };

int mivit_abi_version(void);
const char *mivit_last_error(void);
/* Number of HIP devices visible to the library (0 when there is none); never throws. */
int mivit_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Operator level.  "T" below means the element type selected by `dtype` (float or bf16).
 * ---------------------------------------------------------------------------------------------- */

/* y[M,N] = act(x[M,K] @ W[N,K]^T + bias) (+ resid[M,N]).   nn.Linear + activation
 * (helpers/models.py:37-39,57 q/k/v/out projections; :73-76 FeedForward; :164 patch embedding; :268-273 MLPHead).
 * x is T unless x_is_f32 != 0 (raw fp32 frames for the patch embedding); W, bias fp32; y, resid, y_preact T.
 * y_preact (optional) receives the pre-activation (needed by GELU backward).  ldx/ldy/ldr in elements. */
int mivit_linear_fwd(int dtype, const void *x, int x_is_f32, int64_t ldx, const float *W, const float *bias,
                     int M, int N, int K, int act, const void *resid, int64_t ldr,
                     void *y, int64_t ldy, void *y_preact, void *stream);

/* dx[M,K] = (dy[M,N] @ W[N,K]) (* act'(saved)) (+ dres[M,K]).  Autograd of nn.Linear w.r.t. its input.
 * `act`/`saved`: when act != NONE the result is multiplied by act'(.) evaluated from `saved`[M,K]
 * (post-activation for relu / leaky_relu, PRE-activation for gelu) -- backward of models.py:74. */
int mivit_linear_dgrad(int dtype, const void *dy, int64_t lddy, const float *W, int M, int N, int K,
                       int act, const void *saved, int64_t lds, const void *dres, int64_t lddr,
                       void *dx, int64_t lddx, void *stream);

/* dW[N,K] (+)= dy[M,N]^T @ x[M,K];  db[N] (+)= column sums of dy.  Deterministic (slab split over M, no atomics).
 * workspace: mivit_linear_wgrad_workspace_bytes(M,N,K).  accumulate != 0 adds into dW/db. */
size_t mivit_linear_wgrad_workspace_bytes(int M, int N, int K);
int mivit_linear_wgrad(int dtype, const void *dy, int64_t lddy, const void *x, int x_is_f32, int64_t ldx,
                       int M, int N, int K, float *dW, float *db, int accumulate,
                       void *workspace, size_t workspace_bytes, void *stream);

/* bf16-mode streaming kernels of the frame embedding (LinearProjectionEmbedding / CNNEmbedding, models.py:164,191):
 * the two launches that read the fp32 frames x[M = B*T, K = P*P].  LDS-DMA ring, see csrc/embed.hip.
 *   fwd  : y[M,E] (bf16) = x @ W^T + bias, W given as its bf16 copy [E,K]
 *   wgrad: dW[E,K] (fp32, overwritten) = dy[M,E]^T (bf16) @ x
 * Return 3 when the shape is outside the kernels' constraints (E % 128, K % 128, K >= 256, M >= 128): the caller
 * then uses mivit_linear_fwd / mivit_linear_wgrad, which accept any shape. */
int mivit_embed_fwd_bf16(const float *x, const void *W_bf16, const float *bias, int M, int K, int E, void *y_bf16,
                         void *stream);
/* Forward tiling override (0 = chosen by problem size: embed_fwd_direct2<2,4,3> when M/128 * E/128 >= 512 workgroups,
 * embed_fwd_direct<1,4,3> / <1,2,3> below that; 14 / 8 / 15 force those three, 1 / 2 / 13 the LDS-DMA designs, 3..7 the
 * other direct tilings).  For A/B runs and so that parity tests reach every launcher branch.  Returns the previous value. */
int mivit_embed_set_variant(int variant);
size_t mivit_embed_wgrad_bf16_workspace_bytes(int M, int K, int E);
int mivit_embed_wgrad_bf16(const void *dy_bf16, const float *x, int M, int K, int E, float *dW, void *workspace,
                           size_t workspace_bytes, void *stream);

/* The same two launches for SMALL frames (patch sizes up to 16 x 16 pixels; the shipped configurations use 9 x 9 = 81 and
 * 13 x 13 = 169): x[M, K] fp32 with ANY K <= 256 -- rows are only 4-byte aligned --, E = 64 or 128, M >= 256, M * K * 4 < 2^32.
 * csrc/wavestream.hip (AF32) / csrc/wgrad_small.hip (XF32): the frames are read through a raw buffer at dword alignment and
 * converted in registers.  db (optional) = column sums of dy.  Return 3 outside these constraints. */
int mivit_embed_small_supported(int M, int K, int E);
int mivit_embed_small_fwd(const float *x, const void *W_bf16, const float *bias, int M, int K, int E, void *y_bf16, void *stream);
size_t mivit_embed_small_wgrad_workspace_bytes(int M, int K, int E);
int mivit_embed_small_wgrad(const void *dy_bf16, const float *x, int M, int K, int E, float *dW, float *db, void *workspace,
                            size_t workspace_bytes, void *stream);

/* bf16-mode streaming kernels of the encoder-layer projections (csrc/rowstream.hip, csrc/wgrad_dma.hip): weights are
 * given as bf16 copies, activations are bf16, M = all tokens of the batch.  Return 3 when the shape is outside the
 * kernels' constraints (then use mivit_linear_*).
 *   rowstream_fwd  : y = act(x @ W^T + bias) (+ resid); with ln_gamma != NULL (N == 128, resid given) additionally
 *                    ln_out = LayerNorm(y) and mean/rstd per row -- the post-norm sub-layer of models.py:100-106;
 *   rowstream_dgrad: dx = (dy @ W) (* act'(saved)) (+ dres), W = [N, K] as in mivit_linear_dgrad (at most one of
 *                    saved / dres);
 *   wgrad_bf16     : dW[N, K] (fp32, overwritten) = dy[M, N]^T @ x[M, K]; db[N] (optional) = column sums of dy, taken
 *                    from the same LDS tiles. */
int mivit_rowstream_fwd(const void *x, int64_t ldx, const void *W_bf16, const float *bias, int M, int N, int K, int act,
                        const void *resid, int64_t ldr, void *y, int64_t ldy, void *y_preact, const float *ln_gamma,
                        const float *ln_beta, void *ln_out, float *mean, float *rstd, void *stream);
int mivit_rowstream_dgrad(const void *dy, int64_t lddy, const void *W_bf16, int M, int N, int K, int act,
                          const void *saved, int64_t lds, const void *dres, int64_t lddr, void *dx, int64_t lddx,
                          void *stream);
/* Same contracts as mivit_rowstream_fwd / _dgrad, "wave-stream" data movement (weight slice copied to LDS once, every
 * wave streams its own 16-row tiles straight from global memory into MFMA operands, wave-private epilogue, no barriers);
 * contraction length 128 or 256.  The engine picks per launch whichever of the two measured faster. */
int mivit_wavestream_fwd(const void *x, int64_t ldx, const void *W_bf16, const float *bias, int M, int N, int K, int act,
                         const void *resid, int64_t ldr, void *y, int64_t ldy, void *y_preact, const float *ln_gamma,
                         const float *ln_beta, void *ln_out, float *mean, float *rstd, void *stream);
int mivit_wavestream_dgrad(const void *dy, int64_t lddy, const void *W_bf16, int M, int N, int K, int act,
                           const void *saved, int64_t lds, const void *dres, int64_t lddr, void *dx, int64_t lddx,
                           void *stream);
/* Which launches mivit_rowstream_fwd / _dgrad (and the engine) hand to the wave-stream kernels: 0 = never, 1 = whenever
 * wave-stream supports the shape, 2 = the measured picks (default; initial value from MIVIT_WAVESTREAM).  In mode 2 the mask
 * (initial value from MIVIT_WAVESTREAM_MASK, default 7) enables them one by one: bit 0 the K = 128 forward with fused
 * LayerNorm, bit 1 the K = 128 dgrad with act'(saved), bit 2 every K = 256 dgrad.  For A/B runs and so that tests reach the
 * row-stream kernels behind the picks.  Each returns the previous value. */
int mivit_rowstream_set_wavestream(int mode);
int mivit_rowstream_set_wavestream_mask(int mask);

/* Wide layers (K, N of 512-class models), bf16: LDS-DMA ring GEMMs with 256 x 128 workgroup tiles.
 * fwd:   y = act(x W^T + bias) (+ resid), optional pre-activation copy;   dgrad: dx = (dy W) * act'(saved) (+ dres).
 * N (fwd) / K (dgrad) multiple of 128, contraction length multiple of 64, M >= 256; returns 3 otherwise. */
int mivit_gemm_dma_supported(int M, int N, int K, int dgrad);
/* Tile variant of the sizing sweep (BASELINE config 4's "MFMA tile + LDS sizing"; table in DESIGN.md 4a): 0 = default,
 * 19 = first-generation 8 x (32 x 128) tile, 20..27 = transposed-product tiles.  Returns the previous value. */
int mivit_gemm_dma_set_variant(int variant);
int mivit_gemm_dma_fwd(const void *x, int64_t ldx, const void *W_bf16, const float *bias, int M, int N, int K, int act,
                       const void *resid, int64_t ldr, void *y, int64_t ldy, void *y_preact, void *stream);
int mivit_gemm_dma_dgrad(const void *dy, int64_t lddy, const void *W_bf16, int M, int N, int K, int act,
                         const void *saved, int64_t lds, const void *dres, int64_t lddr, void *dx, int64_t lddx,
                         void *stream);
size_t mivit_wgrad_bf16_workspace_bytes(int M, int N, int K);
int mivit_wgrad_bf16(const void *dy, int64_t lddy, const void *x, int64_t ldx, int M, int N, int K, float *dW, float *db,
                     void *workspace, size_t workspace_bytes, void *stream);
/* Ring configuration of mivit_wgrad_bf16: 0 = by size (default; initial value from MIVIT_WGRAD_DMA_CFG), otherwise
 * 10 * ring slots + rows per stage / 32: 21, 22, 31, 32.  Returns the previous value. */
int mivit_wgrad_bf16_set_config(int cfg);

/* The streaming operators above in IEEE half: csrc/rowstream.hip, wavestream.hip, wgrad_dma.hip, wgrad_small.hip and embed.hip
 * compiled with -DMIVIT_ELEM_F16 export the same entries suffixed _f16 (the engine's fp16 models run on these kernels).  Same
 * arguments with every 16-bit tensor in fp16; the setters act on the fp16 build's own switches. */
int mivit_rowstream_fwd_f16(const void *x, int64_t ldx, const void *W_f16, const float *bias, int M, int N, int K, int act,
                            const void *resid, int64_t ldr, void *y, int64_t ldy, void *y_preact, const float *ln_gamma,
                            const float *ln_beta, void *ln_out, float *mean, float *rstd, void *stream);
int mivit_rowstream_dgrad_f16(const void *dy, int64_t lddy, const void *W_f16, int M, int N, int K, int act,
                              const void *saved, int64_t lds, const void *dres, int64_t lddr, void *dx, int64_t lddx,
                              void *stream);
int mivit_wavestream_fwd_f16(const void *x, int64_t ldx, const void *W_f16, const float *bias, int M, int N, int K, int act,
                             const void *resid, int64_t ldr, void *y, int64_t ldy, void *y_preact, const float *ln_gamma,
                             const float *ln_beta, void *ln_out, float *mean, float *rstd, void *stream);
int mivit_wavestream_dgrad_f16(const void *dy, int64_t lddy, const void *W_f16, int M, int N, int K, int act,
                               const void *saved, int64_t lds, const void *dres, int64_t lddr, void *dx, int64_t lddx,
                               void *stream);
int mivit_rowstream_set_wavestream_f16(int mode);
int mivit_rowstream_set_wavestream_mask_f16(int mask);
size_t mivit_wgrad_bf16_workspace_bytes_f16(int M, int N, int K);
int mivit_wgrad_bf16_f16(const void *dy, int64_t lddy, const void *x, int64_t ldx, int M, int N, int K, float *dW, float *db,
                         void *workspace, size_t workspace_bytes, void *stream);
int mivit_wgrad_bf16_set_config_f16(int cfg);
size_t mivit_wgrad_small_workspace_bytes_f16(int M, int N, int K);
int mivit_wgrad_small_f16(const void *dy, int64_t lddy, const void *x, int64_t ldx, int M, int N, int K, float *dW,
                          float *db, void *workspace, size_t workspace_bytes, void *stream);
int mivit_embed_small_supported_f16(int M, int K, int E);
int mivit_embed_small_fwd_f16(const float *x, const void *W_f16, const float *bias, int M, int K, int E, void *y_f16, void *stream);
size_t mivit_embed_small_wgrad_workspace_bytes_f16(int M, int K, int E);
int mivit_embed_small_wgrad_f16(const void *dy_f16, const float *x, int M, int K, int E, float *dW, float *db, void *workspace,
                                size_t workspace_bytes, void *stream);
int mivit_embed_fwd_bf16_f16(const float *x, const void *W_f16, const float *bias, int M, int K, int E, void *y_f16,
                             void *stream);
int mivit_embed_set_variant_f16(int variant);
size_t mivit_embed_wgrad_bf16_workspace_bytes_f16(int M, int K, int E);
int mivit_embed_wgrad_bf16_f16(const void *dy_f16, const float *x, int M, int K, int E, float *dW, void *workspace,
                               size_t workspace_bytes, void *stream);

/* Fused forward of the two halves of the post-norm encoder layer (helpers/models.py:97-108), bf16 mode, model width
 * E = 128, feed-forward width F = 256, 4 heads of 32 (the PSFNoise 32x64x64 configuration); csrc/fused_fwd.hip.
 * (The reference's shipped width E = 64 / F = 128 / 4 heads of 16: the ..._w64 entries further down.)
 * LayerNorm outputs travel NORMALISED: n = (z - mean) * rstd (bf16) with rstd per row (fp32); a consumer applies the
 * producing LayerNorm's affine while loading, x = gamma_in * n_in + beta_in (gamma_in = beta_in = NULL: n_in is x).
 *   attn_block_fwd: z = x + out_proj(softmax(q k^T / sqrt(32)) v), q|k|v = x Wqkv^T + bqkv   (models.py:33-59,100-102)
 *                   one wavefront per sequence of S <= 64 tokens, weights resident in LDS, q/k/v, probabilities and
 *                   the context never leave registers.  ctx [B*S, E] (the out-projection's input) is written for the
 *                   weight gradient.
 *   mlp_block_fwd : z = x + fc2(act(fc1 x))                                                     (models.py:72-77,104-106)
 *                   one wavefront per 32 rows, the hidden activations never leave registers.
 * Both: n_out = LNhat(z) (bf16), rstd[rows] (fp32).  Optional outputs (NULL = skip), for the unfused backward kernels:
 * x_out = gamma_out * n_out + beta_out, z_out, mean, qkv_out [B*S, 3E], h_out / u_out [M, F] (post- / pre-activation).
 * Weights are bf16 copies in the reference's [out, in] layout; biases and LayerNorm vectors fp32.
 * mivit_fused_layer_supported tells whether a model shape can use them. */
int mivit_fused_layer_supported(int dtype, int embed_dim, int hidden_dim, int num_heads, int tokens);
int mivit_attn_block_fwd(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv_bf16,
                         const float *bqkv, const void *Wo_bf16, const float *bo, const float *gamma_out,
                         const float *beta_out, int B, int S, void *ctx, void *n_out, float *rstd, void *x_out,
                         void *z_out, float *mean, void *qkv_out, void *stream);
int mivit_mlp_block_fwd(const void *n_in, const float *gamma_in, const float *beta_in, const void *W1_bf16,
                        const float *b1, const void *W2_bf16, const float *b2, const float *gamma_out,
                        const float *beta_out, int M, int act, void *n_out, float *rstd, void *x_out, void *z_out,
                        float *mean, void *h_out, void *u_out, void *stream);

/* Fused backward of the feed-forward block (autograd of models.py:72-77,104-106 in the layout above), csrc/fused_bwd.hip:
 * in : dy = dL/dx2 [M,E] bf16 (x2 = gamma2 * n2 + beta2), n2 / rstd2 = LN2's normalised output and 1/std, n1 = LN1's
 *      normalised output (the block input is x1 = gamma1 * n1 + beta1), the bf16 weight copies and fc1's bias;
 * out: dx1 = dL/dx1 [M,E] bf16;  dW1 [F,E], db1 [F], dW2 [E,F], db2 [E], dgamma2 [E], dbeta2 [E] fp32 (overwritten).
 * The hidden activations are recomputed; h, dh and the pre-norm gradient never reach HBM (three row reads, one row write).
 * Deterministic (per-workgroup slabs + fixed-order reduction).  workspace: mivit_mlp_block_bwd_workspace_bytes(M). */
size_t mivit_mlp_block_bwd_workspace_bytes(int M);
/* Which kernel runs it: 8 (default) = hidden units split over eight waves, two per SIMD; 4 = the first kernel, four waves each
 * owning a SIMD's whole register file (kept for A/B runs; same results up to the fp32 summation order of the column sums).
 * Returns the previous value. */
int mivit_mlp_block_bwd_set_waves(int waves);
int mivit_mlp_block_bwd(const void *dy, const void *n2, const float *rstd2, const float *gamma2, const void *n1,
                        const float *gamma1, const float *beta1, const void *W1_bf16, const float *b1, const void *W2_bf16,
                        int M, int act, void *dx1, float *dW1, float *db1, float *dW2, float *db2, float *dgamma2,
                        float *dbeta2, void *workspace, size_t workspace_bytes, void *stream);

/* Noise-free rendering of single-particle image sequences from trajectories (the synthetic-data step right before the hot
 * path: helpers/helpersGeneration.py:128-319 trajectories_to_video / trajectory_to_video / gaussian_2d + block_reduce, and the
 * per-PSF variant Experiments/PSFNoise/trainSettingsPSFNoise.py:196-309).  traj_px [N, T, 2] fp32 positions (x, y) in camera
 * pixels; every frame integrates npos consecutive sub-positions (optionally centred on their mean), each a Gaussian of
 * sigma sigmas[i] (fine-grid units, grid `up` times finer than the camera) whose PEAK on the fine grid is rescaled to
 * amp[n, f, p]; the fine frame is mean-pooled up x up.  out [N, nsig, T / npos, P, P] fp32.  Background, Poisson gain and
 * normalisation are element-wise torch ops on the caller's side (helpers/generation.py). */
int mivit_render_frames(const float *traj_px, int N, int T, int npos, const float *sigmas, int nsig, int P, int up,
                        const float *amp, int center, float *out, void *stream);

/* Noise-free rendering of a whole field of view with many particles (csrc/movie.hip): one spot of the reference's image model
 * (helpers/helpersGeneration.py:283-310: Gaussian on the `up` times finer grid, rescaled to its peak there, mean-pooled),
 * extended by linearity to Np particles in one movie.  pos [Np, F * npos, 2] fp32 positions (y, x) = (row, column) in camera
 * pixels with pixel centres at integers -- the convention of the tracking tables, no flip and no unit conversion --, npos
 * sub-positions per frame; amp [Np, F, npos] the intensity of every sub-position; first / last [Np] int32, or both NULL:
 * particle p is rendered in the frames first[p] .. last[p] inclusive (any values; an empty or outside range renders nothing).
 * With u = c up + (up - 1) / 2, g* = rint(u) and dpk = g* - u, the pooled peak-normalised profile of a position c is
 *   prof(i; c) = (1 / up) sum_{k < up} exp(-(((i up + k) - u)^2 - dpk^2) / (2 sigma_hr^2)),
 * and a sub-position adds amp prof(y; c_y) prof(x; c_x) to the pixels with |y - rint(c_y)| <= radius and
 * |x - rint(c_x)| <= radius, nothing elsewhere.  For odd P up this is mivit_render_frames (center = 0) on a P x P field with
 * c = c_ref + (P - 1) / 2, except at the border: the peak is taken on the UNBOUNDED fine grid, so a particle that leaves the
 * field fades out, where the reference (and mivit_render_frames) rescales it to full intensity on the border pixel.
 * movie [F, H, W] fp32: every element is written exactly once (0 where no window reaches), each pixel summed by one thread,
 * particles ascending and sub-positions ascending within a particle, without atomics: bitwise repeatable.  A sub-position
 * whose position or amplitude is not finite, or whose |coordinate| >= 2^30, contributes nothing.  Limits: 0 <= radius <= 64,
 * 1 <= npos <= 256, 1 <= up <= 64, H, W <= 2^24, sigma_hr > 0 with finite 1 / (2 sigma_hr^2), F * ceil(H / 32) * ceil(W / 64)
 * < 2^31.  Arguments are validated before any HIP call; Np = 0 gives a zero movie.  No index value is read from memory, so no
 * input value can make the kernel read or write out of bounds. */
int mivit_render_movie(const float *pos, const float *amp, const int *first, const int *last, int Np, int F, int npos,
                       float sigma_hr, int up, int radius, int H, int W, float *movie, void *stream);

/* The 25 hand-crafted trajectory descriptors of the ImagesFeatures experiment (reference helpers/helpersFeatures.py:448-519
 * compute_diffusion_features and :524-567 compute_features_for_multiple_trajectories, whose frame averaging :555-558 is fused
 * in; Experiments/ImagesFeatures/trainModelsImagesFeatures.py:36-41 calls it per cycle), csrc/features.hip + csrc/trajfeat.h,
 * one thread per trajectory, fp64.  traj [N, T, 2] positions, dtype MIVIT_F32 or MIVIT_F64; frames of npos sub-steps are
 * averaged in that precision (1 <= npos <= T, T / npos <= 1024 frames, a remainder of T % npos sub-steps is ignored);
 * feats [N, 25] fp64 in helpers/features.py feature_names order, NaN where the reference gives NaN (no nan_to_num); avg
 * [N, T / npos, 2] in the input dtype receives the averaged positions (NULL: not written).  The alpha / D / r2 fit restates
 * scipy's bounded 'trf' curve_fit path.  workspace: mivit_trajectory_features_workspace_bytes(N, T, npos).  Arguments are
 * validated before any HIP call; N = 0 is a no-op. */
size_t mivit_trajectory_features_workspace_bytes(int N, int T, int npos);
int mivit_trajectory_features(const void *traj, int dtype, int N, int T, int npos, double dt, double *feats, void *avg,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Richardson-Lucy deconvolution with total-variation regularisation of every frame of a batch in one launch: the Denoising
 * experiment's apply_rl_tv_tensor_iter_list -> richardson_lucy_tv_iter_list (reference helpers/helpersGeneration.py:542-589,
 * :616-632; called from trajs_to_vid_norm_rl :635-660), csrc/deconv.hip, one workgroup per frame.  frames [B, S, H, W] fp32
 * (device), psf [K, K] fp64 (device), snapshots: HOST array of n_snap strictly increasing 0-based iteration indices
 * (1 <= n_snap <= 16); snapshots[n_snap - 1] + 1 iterations run and out [B, n_snap, S, H, W] fp32 receives the estimate
 * after each listed iteration.  1 <= H, W <= 32, 1 <= K <= 15 (even K as fftconvolve 'same' centres it).  Convolutions and
 * division in fp64, estimate and TV gradient in fp32, in the order of the host restatement (helpers/generation.py), with
 * which it agrees bitwise.  Arguments are validated before any HIP call; B * S = 0 is a no-op. */
int mivit_rl_tv_deconvolve(const float *frames, int B, int S, int H, int W, const double *psf, int K, const int *snapshots,
                           int n_snap, float tv_weight, float *out, void *stream);

/* scipy.ndimage.gaussian_filter(frame, sigma, mode='nearest', truncate) of every frame (what ski.filters.gaussian(frame,
 * sigma=0.5) does for a float image, reference helpers/helpersGeneration.py:530), csrc/deconv.hip: in / out [N, H, W] fp32,
 * 1 <= H, W <= 32, separable fp64 passes (axis 0, then axis 1) with replicated borders, radius int(truncate * sigma + 0.5)
 * <= 15, sigma > 0.  N = 0 is a no-op. */
int mivit_gaussian_filter_frames(const float *in, int N, int H, int W, double sigma, double truncate, float *out,
                                 void *stream);

/* Particle detection for a whole movie: the reference's detect_particles (helpers/helpersTracking.py:12-57, per frame two
 * scipy.ndimage.gaussian_filter calls, their difference, skimage.feature.peak_local_max(dog, min_distance, threshold_abs =
 * threshold_percentage * dog.max(), exclude_border=False)), csrc/tracking.hip, four launches whatever F is.
 * movie [F, H, W] fp32 (device); w1 / w2: HOST arrays of r1 + 1 / r2 + 1 fp64 Gaussian weights, w[0] the centre and w[k] the
 * weight at distance k (the caller builds them as scipy's _gaussian_kernel1d does, radius int(4 sigma + 0.5)),
 * 0 <= r1 <= r2 <= 16 and H, W > r2 (one reflection at the border).  Each filter is two separable passes (axis 0, then
 * axis 1) with scipy's 'reflect' borders, fp64 sums in correlate1d's symmetric order, each pass rounded to fp32; dog = g1 - g2
 * in fp32.  A pixel is a candidate when no pixel of its (2 min_distance + 1)^2 window exceeds it and it is strictly greater
 * than threshold_percentage * max(dog of its frame) (one fp32 product); a frame whose pixels are all equal has none.
 * Candidates are ordered by value descending, ties by row-major index ascending, and kept greedily unless an already kept
 * one lies within Chebyshev distance min_distance (1 .. 16).  cap (1 .. 2048) is the capacity per frame, of candidates and
 * of peaks.  out: count [F] int32 peaks kept, n_candidates [F] int32 candidates before spacing (may exceed cap: then the
 * frame's result is incomplete and the caller must raise), coords [F, cap, 2] int32 (y, x), values [F, cap] fp32, dog
 * [F, H, W] fp32 (NULL: not returned; it then lives in the workspace).  Entries beyond count are not written.  workspace:
 * mivit_dog_peaks_workspace_bytes(F, H, W, cap, dog != NULL).  Arguments are validated before any HIP call; F = 0 is a no-op.
 * The movie must be finite. */
size_t mivit_dog_peaks_workspace_bytes(int F, int H, int W, int cap, int store_dog);
int mivit_dog_peaks(const float *movie, int F, int H, int W, const double *w1, int r1, const double *w2, int r2,
                    float threshold_percentage, int min_distance, int cap, int *count, int *n_candidates, int *coords,
                    float *values, float *dog, void *workspace, size_t workspace_bytes, void *stream);

/* Likelihood-ratio particle detection on the photon-counting camera, csrc/detect.hip: an opt-in detector beside
 * mivit_dog_peaks, in two stages.  Both take the movie [F, H, W] fp32 in camera units, the camera scalars of mivit_fit_spots_mle
 * (d = max((adu - offset) / gain, 0) + read_var; gain > 0, read_var >= 0, finite) and e: a HOST array of 2 r + 1 fp64 values,
 * e[k + r] the pixel-integrated Gaussian profile at offset k from a pixel centre (each in (0, 1]), 1 <= r <= 7, H, W > r.  The
 * template is g(dy, dx) = e[dy] e[dx] and the window of a pixel is the in-frame pixels with |dy|, |dx| <= r (clipped).
 *
 * mivit_score_peaks: the score (Rao) statistic of every pixel.  Column pass A = sum e[dy] d, B = sum d over ascending dy, row
 * pass Sgd = sum e[dx] A, Sd = sum B over ascending dx; per axis the count, sum e and sum e^2 of the valid offsets in ascending
 * order, n = ny nx, Sg = gy gx, Sgg = qy qx; mu0 = Sd / n, U = Sgd - mu0 Sg, V = mu0 (Sgg - Sg Sg / n),
 * S = U > 0 && V > 0 ? U U / V : 0, all fp64 in this order without contraction, S stored as fp32.  Candidates by the rule of
 * mivit_dog_peaks with the absolute `threshold` (finite, >= 0) in place of threshold_percentage * max: a maximum of its clipped
 * (2 min_distance + 1)^2 window strictly above the threshold, none in a frame whose pixels are all equal, ordered by value
 * descending and row-major index ascending, kept greedily at Chebyshev distance > min_distance (1 .. 16).  cap (1 .. 2048),
 * count, n_candidates, coords, values and the workspace as mivit_dog_peaks; map [F, H, W] fp32 or NULL (it then lives in the
 * workspace: mivit_score_peaks_workspace_bytes(F, H, W, cap, map != NULL)).
 *
 * mivit_lrt_peaks: the exact Poisson likelihood ratio at the candidates count_in [F] / coords_in [F, cap, 2] / values_in
 * [F, cap] that mivit_score_peaks left.  One wave per frame, one lane per candidate.  Over the window row-major: n, Sd, Sgd,
 * Sg, Sgg, then mu0, U and den = Sgg - Sg Sg / n as above; a candidate without U, den, mu0 > 0 has T = 0.  Otherwise
 * mu_k = theta g_k + beta is fitted by the damped loop of mivit_fit_spots_mle (lambda schedule, slack 1e-13 of 2 sum(mu + d),
 * stopping rule on the undamped step at 1e-11 of max(|theta|, |beta|), 100 iterations) on the 2 x 2 Fisher matrix from
 * theta = U / den, beta = mu0 - theta Sg / n (where that beta is not positive: beta = mu0 / 1000, theta = (Sd - n beta) / Sg);
 * a trial point with theta <= 0 or a pixel with mu <= 0 is rejected.  T = max(0, 2 sum d log(mu / mu0) - 2 (sum mu - Sd)) with
 * 0 log = 0.  A candidate is kept when T > threshold and the kept ones are compacted per frame in their order.  out: count [F]
 * int32, coords [F, cap, 2] int32, stats [F, cap, 4] fp64 (T, photons = theta, background = beta - read_var, the stage-1 S),
 * status [F, cap] int32: 0 converged, 1 damping exhausted, 2 iteration cap (T is then that of the last accepted point, a lower
 * bound).  Entries beyond count are not written; the outputs must not alias the inputs.  A candidate outside the frame is
 * dropped and count_in is read as at most cap.
 *
 * Arguments are validated before any HIP call; F = 0 is a no-op.  The movie must be finite. */
size_t mivit_score_peaks_workspace_bytes(int F, int H, int W, int cap, int store_map);
int mivit_score_peaks(const float *movie, int F, int H, int W, const double *e, int r, double gain, double offset,
                      double read_var, float threshold, int min_distance, int cap, int *count, int *n_candidates, int *coords,
                      float *values, float *map, void *workspace, size_t workspace_bytes, void *stream);
int mivit_lrt_peaks(const float *movie, int F, int H, int W, const double *e, int r, double gain, double offset,
                    double read_var, double threshold, int cap, const int *count_in, const int *coords_in,
                    const float *values_in, int *count, int *coords, double *stats, int *status, void *stream);

/* Sub-pixel localisation: the five-parameter fit inside the reference's add_refined_localization_to_dataframe
 * (helpers/helpersTracking.py:555-604, one scipy.optimize.curve_fit per patch), csrc/tracking.hip, one thread per patch.
 * patches [N, P, P] fp32, P odd, 3 .. 15.  Model offset + amplitude exp(-((x - x0)^2 + (y - y0)^2) / (2 sigma^2)) on the
 * pixel grid 0 .. P-1, start (patch.max(), P / 2, P / 2, 1.0, patch.min()), Levenberg-Marquardt in fp64 with the analytic
 * Jacobian, stopped when every parameter's undamped step is below xtol relative to its scale (0 < xtol <= 1.49012e-8, MINPACK's
 * default) or after 100 iterations.  out: params [N, 5] fp64 (amplitude, x0, y0, sigma, offset), peak [N] fp32 = patch.max(),
 * status [N] int32: 0 converged, 1 damping exhausted, 2 iteration cap, 3 non-finite patch.  The reference's fallback for a
 * failed fit is the caller's business.  Arguments are validated before any HIP call; N = 0 is a no-op. */
int mivit_refine_gaussian(const float *patches, int N, int P, double xtol, double *params, float *peak, int *status,
                          void *stream);

/* Poisson maximum-likelihood fit of every localisation with a Cramer-Rao bound per parameter (Smith et al., Nat. Methods 2010,
 * in the Levenberg-Marquardt form of Laurence & Chromy 2010), csrc/localize.hip, one thread per patch.  patches [N, P, P] fp32,
 * P odd, 3 .. 15, pixel centres at integers.  Data d = max((patch - offset) / gain, 0) + read_var (gain > 0 in ADU per photon,
 * offset in ADU, read_var >= 0 the readout variance in photons^2, added to data and model as Huang et al. 2013 do).  Model
 * mu = b + N E(ix; x0, s) E(iy; y0, s) + read_var with E the Gaussian integrated over the pixel, parameters (N photons, x0, y0,
 * s, b); fit_sigma = 0 holds s at sigma0 (0.2 < sigma0 < P).  The damped loop of mivit_refine_gaussian (same lambda schedule,
 * stopping rule on the undamped step with 0 < xtol <= 1.49012e-8, 100 iterations) on the Poisson deviance
 * 2 sum(mu - d + d log(d / mu)) with the Fisher information sum dmu dmu^T / mu as its matrix; a step is accepted unless the
 * deviance rises by more than 1e-13 of 2 sum(mu + d), the magnitude its rounding error scales with; a trial point with N <= 0,
 * s outside (0.2, P) or a pixel with mu <= 0 is rejected like a cost increase.  Start: b = min(d) but at least 1e-3 max(d),
 * N = max(sum(d - b), max(d)), the centre P / 2, sigma0.  out: params [N, 5] fp64; crlb [N, 5] fp64, the diagonal of the
 * inverse Fisher matrix at the returned point (variances; NaN where status != 0 or the matrix is not positive definite; the s
 * entry is 0 with fit_sigma = 0); deviance [N] fp64; status [N] int32: 0 converged, 1 damping exhausted (or a patch without a
 * photon), 2 iteration cap, 3 non-finite patch (parameters NaN); iterations [N] int32.  Arguments are validated before any
 * HIP call; N = 0 is a no-op. */
int mivit_fit_spots_mle(const float *patches, int N, int P, double gain, double offset, double read_var, double sigma0,
                        int fit_sigma, double xtol, double *params, double *crlb, double *deviance, int *status,
                        int *iterations, void *stream);

/* Joint Poisson maximum-likelihood fit of a localisation and one neighbour inside its patch, csrc/localize2.hip, one wave per
 * patch.  patches [N, P, P] fp32, camera scalars, sigma0, fit_sigma and xtol as mivit_fit_spots_mle.  count [N] int32: the
 * emitters of each patch, 1 or 2; guess [N, 4] fp64: the starting centres x1, y1, x2, y2 in patch coordinates (the last two are
 * not read where count = 1).  Model mu = b + sum_{e < count} N_e E(ix; x_e, s) E(iy; y_e, s) + read_var, one width and one
 * background for both emitters, parameters (N1, x1, y1, N2, x2, y2, s, b).  Start: b and the photons above it as
 * mivit_fit_spots_mle, split evenly between the emitters.  The loop is that of mivit_fit_spots_mle (lambda schedule, stopping
 * rule, cost slack, Fisher information); a trial point with an N_e <= 0, s outside (0.2, P), a centre outside [-1, P] on either
 * axis or a pixel with mu <= 0 is rejected like a cost increase.  out: params [N, 8] fp64; crlb [N, 8] fp64, the diagonal of
 * the inverse Fisher matrix at the returned point (NaN where status != 0 or the matrix is not positive definite, as for two
 * emitters that collapsed onto each other; the s entry is 0 with fit_sigma = 0); where count = 1 the fit is the five-parameter
 * one and the three entries of emitter 2 are NaN in both; deviance [N] fp64; status [N] int32: 0 converged, 1 damping
 * exhausted (or no photon, a starting centre outside [-1, P], or two starting centres on one point: singular by symmetry, no
 * iteration), 2 iteration cap, 3 non-finite patch or guess, or a count
 * that is neither 1 nor 2; iterations [N] int32.  A row with status 3 holds NaN in all eight parameters, in all eight entries
 * of crlb and in deviance, and 0 in iterations; count is only compared with 1 and 2, so no value of it can address anything.
 * Every sum is taken by one lane in pixel order: the result of a patch does not depend on the batch, nor on the rows around
 * it.  Arguments are validated before any HIP call; N = 0 is a no-op. */
int mivit_fit_spots_mle2(const float *patches, const int *count, const double *guess, int N, int P, double gain, double offset,
                         double read_var, double sigma0, int fit_sigma, double xtol, double *params, double *crlb,
                         double *deviance, int *status, int *iterations, void *stream);

/* The nearest other detection of the same frame for every row of a detections table sorted by frame, csrc/localize2.hip, one
 * thread per row.  frame_offsets [F + 1] int32: rows frame_offsets[f] .. frame_offsets[f + 1] - 1 belong to frame f (clamped to
 * 0 .. n); ys, xs [n] int32 the integer positions; reach >= 0.  out: neighbour [n] int32, the row of the same frame with
 * max(|dy|, |dx|) <= reach that is nearest by squared Euclidean distance, ties to the lower row, -1 if there is none;
 * n_neighbours [n] int32, the number of rows within reach.  frame_offsets must ascend from 0 to n (only its first entry may
 * lie below 0 and its last above n: they count as 0 and n).  For offsets that do not ascend or do not cover 0 .. n no frames
 * are defined, and all a caller may rely on is that nothing outside the five arrays is read or written, that every entry of
 * both outputs is written, that neighbour[i] is -1 or a row in [0, n) and that n_neighbours[i] lies in [0, n).  Arguments are
 * validated before any HIP call; n = 0 is a no-op. */
int mivit_spot_neighbours(const int *frame_offsets, const int *ys, const int *xs, int F, int n, int reach, int *neighbour,
                          int *n_neighbours, void *stream);

/* Linking of a whole movie: the reference's link_particles (helpers/helpersTracking.py:123-177, one
 * scipy.optimize.linear_sum_assignment per frame) for all F - 1 pairs of consecutive frames in one launch, csrc/linking.hip.
 * coords [F, cap, 2] int32 (y, x) and count [F] int32 as mivit_dog_peaks leaves them (device); movie_start [F] bytes or NULL:
 * a non-zero entry marks the first frame of a movie, which gets no links (frame 0 always is one).  Per frame f the full
 * rectangular assignment between the detections of f - 1 and of f is solved exactly on the Euclidean distance (shortest
 * augmenting paths with duals, fp64; the side with fewer detections plays rows, f - 1 on equality; ties by path cost, then
 * free column first, then column index), and only then links longer than max_distance are dropped.  out: link [F, cap] int32,
 * for every detection of frame f the index of its partner in frame f - 1 or -1; every entry is written.  1 <= cap <= 1024.
 * Arguments are validated before any HIP call; F = 0 is a no-op, empty frames are valid. */
int mivit_link_frames(const int *coords, const int *count, const unsigned char *movie_start, int F, int cap,
                      double max_distance, int *link, void *stream);

/* Track ids from the links: the book-keeping of the reference's track_particles (helpers/helpersTracking.py:225-336),
 * csrc/linking.hip, one workgroup looping over the frames.  A linked detection inherits its partner's id, an unlinked one takes
 * the next free id in ascending detection index; frame 0 and every movie_start frame start one track per detection.  out: ids
 * [F, cap] int32 (entries beyond count[f] are not written), lengths [>= number of tracks; F * cap always suffices] int32,
 * the number of positions of each track, n_tracks [1] int32.  1 <= cap <= 1024.  Arguments are validated before any HIP call;
 * F = 0 only clears n_tracks. */
int mivit_chain_tracks(const int *link, const int *count, const unsigned char *movie_start, int F, int cap, int *ids,
                       int *lengths, int *n_tracks, void *stream);

/* Gap closing: the end of a track is linked to the start of a later track across up to max_gap missed frames (1 .. 8),
 * csrc/linking.hip.  coords / count / movie_start as for mivit_link_frames, link [F, cap] as it wrote it (a value outside
 * 0 .. count[f - 1] - 1 counts as -1).  An open start is a detection without a link and without a gap link, an open end one
 * that no detection of the next frame links to and no gap link points at.  Passes g = 2 .. max_gap + 1, one launch each of F
 * one-wave workgroups: workgroup f solves the full rectangular assignment between the open ends of frame f - g and the open
 * starts of frame f, both in ascending detection index, with the solver, roles and tie rule of mivit_link_frames, then drops
 * the pairs longer than max_distance; an accepted pair closes both ends, a dropped one leaves them open for the later passes.
 * A pair of frames is skipped when f - g < 0 or one of the frames f - g + 1 .. f carries a movie_start flag.  out: gap_partner
 * [F, cap] int32, the index in frame f - g or -1, gap_frames [F, cap] int32, g or 0; every entry is defined (the first launch
 * clears both, a pass overwrites an entry at most once).  workspace: workspace_bytes >= F * cap bytes on the device, the
 * open-end state.  1 <= cap <= 1024.  Arguments are validated before any HIP call; F = 0 is a no-op. */
int mivit_close_gaps(const int *coords, const int *count, const int *link, const unsigned char *movie_start, int F, int cap,
                     int max_gap, double max_distance, int *gap_partner, int *gap_frames, unsigned char *workspace,
                     size_t workspace_bytes, void *stream);

/* mivit_chain_tracks with gap links: a detection with a link inherits the id of its partner in frame f - 1, otherwise one with
 * gap_frames = g in 2 .. max_gap + 1 the id of detection gap_partner of frame f - g, otherwise it takes the next free id; frame
 * 0 and every movie_start frame start one track per detection.  A link or gap partner outside the partner frame's count, or a
 * g outside 2 .. max_gap + 1 or beyond frame 0, counts as absent.  out: ids [F, cap] int32 (entries beyond count[f] are not
 * written), lengths [F * cap] int32, cleared here, the number of DETECTIONS of each track, n_tracks [1] int32.
 * 1 <= max_gap <= 8, 1 <= cap <= 1024.  Arguments are validated before any HIP call; F = 0 only clears n_tracks. */
int mivit_chain_tracks_gaps(const int *link, const int *gap_partner, const int *gap_frames, const int *count,
                            const unsigned char *movie_start, int F, int cap, int max_gap, int *ids, int *lengths,
                            int *n_tracks, void *stream);

/* Ragged mean square displacement and both classical estimates of the diffusion coefficient for every track of a linked
 * movie in one launch (the reference's mean_square_displacement, helpers/helpersMSD.py:7-26, estimateDfromMSDs, :110-129, and
 * estimateDfromMSDsWeighted, :131-157, per track), csrc/diffusion.hip, one workgroup per track, one thread per lag.
 * pos [N, 2] fp64 sorted by track and by frame within a track; offsets [n_tracks + 1] int32 (CSR); a lag in rows is a lag in
 * frames (tracks have no gaps).  Per track of L rows, M = L - 1, or min(L - 1, max_lag) with max_lag > 0:
 *   msd[tau] = (sum_{i ascending} (dy * dy + dx * dx)) / (L - tau) for tau = 1 .. M, every other entry of the row 0;
 *   d_lstsq = (sum_tau (tau dt) msd[tau]) / (sum_tau (tau dt)^2) / 4, the line through the origin;
 *   d_weighted = (sum_tau (msd[tau] / tau) (M + 1 - tau)) / ((M + 1)(M + 2) / 2) / 4: the weight sum includes lag 0 and the lag
 *   is counted in steps, as in the reference;
 * all sums in ascending index in fp64 without contraction, so the result is independent of the launch geometry.  M < 1 gives a
 * zero row and NaN for both estimates.  out: msd [n_tracks, Lmax] fp64 (every entry written; Lmax >= the longest track, lags
 * beyond Lmax - 1 are not computed), d_lstsq / d_weighted [n_tracks] fp64.  Tracks of up to 4096 rows are staged in LDS.
 * Arguments are validated before any HIP call; n_tracks = 0 is a no-op. */
int mivit_track_msd(const double *pos, int N, const int *offsets, int n_tracks, double dt, int max_lag, int Lmax, double *msd,
                    double *d_lstsq, double *d_weighted, void *stream);

/* The model's input from the detections table in one launch: the reference's extract_particle_patches
 * (helpers/helpersTracking.py:513-550) followed by normalize_images (helpers/helpersGeneration.py:356-400), cut into windows of
 * T rows, csrc/diffusion.hip, one thread per output element.  movie [F, H, W] fp32; frame / y / x [N] int32 per table row
 * (positions already rounded); seq_row [n_seq] int32, the row where each window starts; P odd, 3 .. 15.  out: seq
 * [n_seq, T, P, P] fp32, patch t of window s centred on row seq_row[s] + t; pixels outside the frame read as 0 BEFORE the
 * normalisation (v - lo) / denom (IEEE fp32 division; skipped with normalize = 0).  A row outside [0, N) or with a frame
 * outside [0, F) gives a zero patch: nothing is read out of bounds whatever the index values are.  Arguments are validated
 * before any HIP call; n_seq = 0 is a no-op. */
int mivit_track_sequences(const float *movie, int F, int H, int W, const int *frame, const int *y, const int *x, int N,
                          const int *seq_row, int n_seq, int T, int P, float lo, float denom, int normalize, float *seq,
                          void *stream);

/* Fractional Gaussian noise, the increments of anomalous diffusion with MSD ~ t^alpha (the displacement law of the reference's
 * disp_fbm, Experiments/mitochondria_simulation/mitochnodria.py:436-476, which draws them from the `fbm` package), csrc/fbm.hip,
 * one workgroup per trajectory.  z [N, T, C] fp64 standard normals, 1 <= C <= 4 axes that share one exponent; gamma [U, T] fp64,
 * one autocovariance row per distinct exponent, gamma[k] = (|k+1|^alpha - 2 |k|^alpha + |k-1|^alpha) / 2 computed by the caller
 * (helpers/generation.fgn_autocovariance: no device pow); gamma_row [N] int32 in [0, U) names each trajectory's row (an entry
 * outside is clamped: nothing is read out of bounds).  out [N, T, C] fp64 = L z per trajectory and axis, L the lower Cholesky
 * factor of the T x T Toeplitz matrix of gamma, by the Durbin-Levinson recursion with all three sums of a step taken on the
 * previous step's coefficients (v_0 = gamma[0], g_0 = sqrt(v_0) z_0, phi empty):
 *   A = sum_j phi[j] gamma[n-j],  B = sum_j phi[j] g[n-j],  R = sum_j phi[n-j] g[n-j],  j = 1 .. n-1
 *   kappa = (gamma[n] - A) / v;  v = v (1 - kappa^2);  g[n] = ((B - kappa R) + kappa g[0]) + sqrt(v) z[n]
 *   phi[j] = phi[j] - kappa phi[n-j] (j < n),  phi[n] = kappa
 * in fp64 without contraction; lane j mod 256 owns term j and the partial sums go through one fixed tree, so a trajectory's
 * result is bitwise the same alone, in any batch and in every launch.  gamma = (1, 0, 0, ...) (alpha = 1) returns z.
 * T <= 2048 (gamma, phi and the C histories live in LDS, (2 + C) T doubles); a larger T is an error, never a launch.
 * Arguments are validated before any HIP call; N = 0 or T = 0 is a no-op. */
int mivit_fgn(const double *z, const double *gamma, const int *gamma_row, int N, int T, int C, int U, double *out, void *stream);

/* Confined diffusion on filament geometries: 1-D displacements along a polyline become 2-D positions (the reference's
 * Geometry.map_displacements, Experiments/mitochondria_simulation/mitochnodria.py:339-378, with get_edge_at_length, :231-264,
 * and Edge.get_position_at_distance, :87-102), csrc/confine.hip, one workgroup per particle, one launch.
 * disp [N, T] fp64 steps along the filament, s0 [N] fp64 start arcs, geom_of [N] int32 in [0, G).  The G polylines are packed
 * by the caller (helpers/geometry.pack_geometries, the one host function: no device sqrt): verts [V, 2] fp64, vert_offsets
 * [G + 1] int32 (geometry g owns vertices vert_offsets[g] .. vert_offsets[g + 1] - 1 and one edge fewer), lengths [V] fp64
 * (lengths[v] = |verts[v + 1] - verts[v]|, the last slot of a geometry unused), totals [G] fp64.  With L = totals[geom_of[n]]:
 *   clamp(m): m = (L < m) ? L : m;  m = (m > 0) ? m : 0                 (Python's max(0, min(m, L)); NaN -> 0)
 *   mode 0, clamp (the reference):  s = clamp(s0);  per step s = clamp(s + d[t])
 *   mode 1, reflect:  fold(m): P = 2 L; m = fmod(m, P); if (m < 0) m = m + P; if (m > L) m = P - m; m = clamp(m)
 *                     s = fold(s0);  per step s = fold(s + d[t])        (per step on the position, not on the free sum)
 *   lookup: rem = s; the first edge e in order with rem <= lengths[e] is the edge (the earlier one at a vertex), otherwise
 *   rem = rem - lengths[e]; pos = verts[e] + (clamp of rem to [0, lengths[e]] / lengths[e]) * (verts[e + 1] - verts[e]); no edge
 *   found (the remainder ends a few ulps above the last length): pos = the last vertex, edge = the last edge
 * in fp64 without contraction, the steps of a particle walked in ascending t by one thread, so a particle's result is bitwise
 * the same alone, in any batch and in every launch, and bitwise that of the numpy restatement (helpers/geometry).
 * out: pos [N, T, 2] fp64 (the vertex components in the order given), arc [N, T] fp64 (s after step t) or NULL, edge [N, T] int32
 * (index within the geometry) or NULL.  No limit on T.  A geometry has at most 512 edges (it is staged in LDS); geom_of and
 * vert_offsets are clamped before use, so nothing is read out of bounds whatever they hold, and sizes that prove a longer
 * polyline are an error, never a launch.  The rule: g = geom_of[n] clamped to [0, G - 1]; v0 = vert_offsets[g] clamped to
 * [0, V - 2]; v1 = vert_offsets[g + 1] raised to v0 + 2 if it is smaller, otherwise lowered to V if it is larger; the particle
 * walks the polyline of the vertices v0 .. v1 - 1 with the edge lengths lengths[v0 .. v1 - 2], of which the first 512 edges
 * are used, with L = totals[g] as stored (a total beyond the polyline that is left ends in "no edge found").  For packed
 * geometries this changes nothing.  Arguments are validated before any HIP call; N = 0 or T = 0 is a no-op. */
int mivit_map_displacements(const double *disp, const double *s0, const int *geom_of, const double *verts, const double *lengths,
                            const int *vert_offsets, const double *totals, int N, int T, int G, int V, int mode, double *pos,
                            double *arc, int *edge, void *stream);

/* Multi-state diffusion, csrc/segment.hip: tracks whose diffusion coefficient changes (andi_datasets' multi_state, from whose
 * single_state the reference takes its trajectories; no counterpart in the reference itself).  All three in fp64 without
 * contraction, no atomics, a track's / segment's / particle's result bitwise the same alone, in any batch and in every launch.
 *
 * mivit_segment_tracks: the optimal partition of every track into stretches of constant step variance, one wave per track.
 * pos [N, 2] fp64 sorted by track and by frame, offsets [n_tracks + 1] int32 (CSR; entries are clamped to [0, N]: nothing is
 * read out of bounds), max_len >= the rows of the longest track and <= 4096 (cs, F and prev live in LDS, 20 B a row; a larger
 * value is an error, never a launch, and a track that is longer than max_len after all is cut to it).  A track of L rows has
 * Linc = L - 1 increments, q_k = dy_k^2 + dx_k^2 between rows k and k + 1, cs[j] = q_0 + .. + q_{j-1} summed in ascending k
 * (np.cumsum bit for bit), and with n = j - i, beta = penalty * log(Linc):
 *   C(i, j) = (2 n) * log(max((cs[j] - cs[i]) / (2 n), min_var))        -2 log L of 2 n Gaussian samples, up to a constant
 *   F(0) = -beta;  F(j) = min over i in {0} and [min_len, j - min_len] of (F(i) + C(i, j)) + beta,   j = min_len .. Linc
 * prev[j] is the LOWEST i among equal minima; backtracking prev from Linc gives the changepoints.  Linc < 2 min_len leaves
 * only i = 0: no changepoint; 1 <= Linc < min_len has no step of the recurrence and gets F(Linc) = (F(0) + C(0, Linc)) + beta.
 * out: seg_start [N] int32, 1 on the first row of every segment (a track's first row included; a changepoint at increment c
 * puts the shared row c into the later segment), 0 elsewhere on a track's rows; cost [n_tracks] fp64 = F(Linc), NaN where
 * Linc < 1.  The only operation that may differ from the numpy restatement (helpers/msd._segment_numpy) is log.
 * min_len >= 2, penalty >= 0, min_var > 0.  Arguments are validated before any HIP call; n_tracks = 0 is a no-op.
 *
 * mivit_segment_stats: one row of estimates per segment, one thread per segment.  seg_offsets [n_seg + 1] int32, the CSR of
 * the segments over the same rows; seg_track_end [n_seg] int32, the row at which each segment's track ends (exclusive).  The
 * increments of segment s run from row seg_offsets[s] to row min(seg_offsets[s + 1], seg_track_end[s] - 1): the increment that
 * bridges to the next segment belongs to the earlier one; n is their number.  Sums in ascending index:
 *   S2 = sum_k q_k;   S11 = sum_k (dy_k dy_{k+1} + dx_k dx_{k+1}) over the n - 1 neighbouring pairs inside the segment
 *   D_mle  = S2 / ((4 n) dt)
 *   D_cve  = D_mle + S11 / ((2 (n - 1)) dt)                             Vestergaard et al. 2014: localisation noise and
 *   sigma2 = (R S2) / (2 n) + ((2 R - 1) S11) / (2 (n - 1))             motion blur (coefficient R in [0, 1/4]) cancel
 * NaN where a divisor is below 1 (D_mle: n < 1; D_cve, sigma2: n < 2); n_increments [n_seg] int32.  No log: bitwise the numpy
 * restatement (helpers/msd._segment_stats_numpy).  Rows are clamped to [0, N - 1].  dt > 0.  n_seg = 0 is a no-op.
 *
 * mivit_markov_states: the state path of every particle of a K-state Markov chain, one thread per particle.  u [N, T] fp64
 * uniforms, p0 [K] and M [K, K] fp64 (rows summing to 1), 1 <= K <= 8.  state[n, 0] is the first k with u[n, 0] < p0[0] + ..
 * + p0[k], the cumulative sum taken sequentially, and K - 1 if there is none (rounding); state[n, t] the same on row
 * M[state[n, t - 1]].  out: state [N, T] int32.  Adds and compares only: bitwise the numpy restatement
 * (helpers/generation._markov_host).  N = 0 or T = 0 is a no-op. */
int mivit_segment_tracks(const double *pos, int N, const int *offsets, int n_tracks, int max_len, int min_len, double penalty,
                         double min_var, int *seg_start, double *cost, void *stream);
int mivit_segment_stats(const double *pos, int N, const int *seg_offsets, const int *seg_track_end, int n_seg, double dt,
                        double R, double *d_cve, double *d_mle, double *sigma2, int *n_increments, void *stream);
int mivit_markov_states(const double *u, const double *p0, const double *M, int N, int T, int K, int *state, void *stream);

/* Diffusion states shared across tracks, csrc/hmm.hip: a hidden Markov model over the increments of ALL tracks of a movie, the
 * inverse of multi_state above (K variances and K x K transition probabilities pooled over every row; the maximum-likelihood
 * form of vbSPT; no counterpart in the reference).  fp64 without contraction, no LDS, no atomics; a group of 8 lanes owns a
 * track and lane j is state j (a 64-thread workgroup holds 8 tracks); a track's outputs are bitwise the same alone, anywhere
 * in a batch and in every launch.  A track has NO maximum length: the recurrence's state lives in global memory.
 *
 * pos [N, 2] fp64 sorted by track and by frame, offsets [n_tracks + 1] int32 (CSR; entries are clamped to [0, N]: nothing is
 * read or written out of bounds whatever they hold).  A track of L rows at rows a .. a + L - 1 has T = L - 1 increments,
 * q_t = dy_t^2 + dx_t^2 between rows t and t + 1.  1 <= K <= 8 states; state j has the per-axis increment variance v[j]
 * (= 2 D_j dt + 2 sigma2 for the caller; the correlation that localisation noise puts between neighbouring increments is
 * ignored), A [K, K] the transition probabilities, pi [K] the initial distribution.  With v_max = max_j v[j]:
 *   m_t = q_t / (2 v_max);   b_j(q_t) = exp(-(q_t / (2 v_j) - m_t)) / v_j       exponent <= 0, the widest state has exp(0)
 * (the density of the increment is b_j exp(-m_t) / (2 pi)).
 *
 * mivit_hmm_estep: the scaled forward-backward pass.  Every sum over a state index starts at 0 and runs in ascending index;
 * t ascends in the forward pass and descends in the backward pass (the statistics are summed in descending t):
 *   x_0 = pi * b(q_0);   x_t[j] = (sum_i alpha_{t-1}[i] * A[i][j]) * b_j(q_t);   c_t = sum_j x_t[j];   alpha_t = x_t / c_t
 *   beta_{T-1} = 1;   w_{t+1}[j] = (b_j(q_{t+1}) / c_{t+1}) * beta_{t+1}[j];   beta_t[i] = sum_j A[i][j] * w_{t+1}[j]
 *   gamma_t = alpha_t * beta_t;   xi_t[i][j] = (alpha_t[i] * A[i][j]) * w_{t+1}[j]      (t = 0 .. T - 2)
 * out, per track: xi [n_tracks, K, K] = sum_t xi_t; g_sum [n_tracks, K] = sum_t gamma_t; gq_sum [n_tracks, K] = sum_t gamma_t
 * * q_t; g_first [n_tracks, K] = gamma_0; loglik [n_tracks] = (sum_t log c_t - sum_t m_t) - T * log(2 pi), the two sums in
 * ascending t.  out, per row: gamma [N, K], row a + t holds increment t and the last row of a track repeats the row before it;
 * state [N] int32, the LOWEST index among the largest gamma.  A track with T < 1 has NaN statistics and loglik (a one-row
 * track NaN in its gamma row and state -1).  The first c_t that is not in (0, inf) ends a track: loglik = -inf where that
 * c_t is 0 (the likelihood underflowed under these parameters), NaN otherwise (a NaN or infinite position), and all its
 * statistics and gamma rows are NaN, its states -1; no other track is touched.  workspace: [N, K] fp64 (b / c_t).  alpha_t is
 * kept in gamma on the way forward; a lane reads back only what it wrote itself.  The only operations that may differ from
 * the numpy restatement (helpers/msd._hmm_estep_numpy) are exp and log.
 *
 * mivit_hmm_viterbi: the most probable state path, in the log domain with every logarithm taken by the caller: logv [K] =
 * log v, logA [K, K] = log A, logpi [K] = log pi (-inf where the probability is 0).
 *   lb_j(q) = -(q / (2 v_j)) - logv_j;   delta_0[j] = logpi[j] + lb_j(q_0)
 *   delta_t[j] = max_i (delta_{t-1}[i] + logA[i][j]) + lb_j(q_t),   the LOWEST i among equal maxima is the back-pointer
 * (a candidate replaces the running maximum only where it compares greater, so NaN candidates never do); the path ends in the
 * lowest j among the largest delta_{T-1} and follows the back-pointers.  out: state [N] int32 (row a + t = increment t, the
 * last row repeats, -1 for a one-row track), logp [n_tracks] fp64 = max_j delta_{T-1}[j] (NaN where T < 1).  workspace:
 * [N, 8] bytes, the back-pointers.  Adds, one division and compares only: bitwise the numpy restatement
 * (helpers/msd._hmm_viterbi_numpy).
 *
 * Both: arguments are validated before any HIP call (sizes, K, null pointers); n_tracks = 0 is a no-op. */
int mivit_hmm_estep(const double *pos, int N, const int *offsets, int n_tracks, int K, const double *v, const double *A,
                    const double *pi, double *gamma, int *state, double *xi, double *g_sum, double *gq_sum, double *g_first,
                    double *loglik, double *workspace, void *stream);
int mivit_hmm_viterbi(const double *pos, int N, const int *offsets, int n_tracks, int K, const double *v, const double *logv,
                      const double *logA, const double *logpi, int *state, double *logp, unsigned char *workspace, void *stream);

/* Stage drift, csrc/drift.hip: the motion all tracks of a movie share, from their frame-to-frame increments (trackpy's
 * compute_drift; no counterpart in the reference, whose movies do not drift).  fp64 without contraction, no atomics; a frame's
 * result is bitwise the same alone, in any batch and in every launch, and bitwise the numpy restatements' (helpers/msd.
 * _drift_frames_numpy, _drift_integrate_numpy): adds, multiplications, divisions and compares only.
 *
 * mivit_drift_frames: one statistic of the increments per frame and axis, ONE WORKGROUP of 256 threads per frame.  pos [N, 2]
 * fp64, the table sorted by track; pair_row [M] int32: increment m is pos[r] - pos[r - 1] with r = pair_row[m], gathered by
 * the kernel (r is clamped to [1, N - 1]: nothing is read out of bounds; M > 0 needs N >= 2); frame_offsets [F + 1] int32, the
 * CSR of pair_row over the frames (entries clamped to [0, M]); the increments of frame f are d_0 .. d_{n-1} in the order of
 * pair_row.  out: stat [F, 2] fp64, 0 where n = 0.
 *   mode 0, mean:   s_t = ((+0 + d_t) + d_{t+256}) + d_{t+512} + ..   for t = 0 .. 255 (+0 where the frame has no such entry);
 *                   then for half = 128, 64, .. 1:  s_i = s_i + s_{i+half}, i < half;   stat = s_0 / n.
 *                   The order depends on the position of an increment within its frame alone; n has no limit.
 *   mode 1, median: per axis the exact median under the order of the values with -0 before +0: the middle value for odd n,
 *                   (a + b) / 2 of the two middle values for even n; NaN if an increment of the axis is NaN.  The frame is
 *                   sorted in LDS (a bitonic network over 64-bit keys, 8 B a pair, padded to a power of two), so n <= 4096
 *                   (32 KiB: five workgroups a CU); max_pairs >= the pairs of the largest frame sizes the LDS of the launch, a
 *                   value above 4096 is an error, never a launch, and a frame that is larger after all is cut to its first
 *                   increments, as many as the LDS of the launch holds.  max_pairs is not used by mode 0.
 *
 * mivit_drift_integrate: stat [F, 2], n_pairs [F] int32 (the weights: the pairs of each frame, negative counts as 0),
 * half_window h >= 0 -> velocity [F, 2], drift [F, 2] fp64.  With W(f) = [max(1, f - h), min(F - 1, f + h)]:
 *   velocity[f] = (sum_{g in W(f)} n_g * stat_g) / (sum_{g in W(f)} n_g)   the numerator from +0 in ascending g, the product
 *                 rounded before it is added, the denominator in integers; 0 where the denominator is 0
 *   velocity[0] = 0;   h = 0: velocity[f] = stat[f] itself, bit for bit, for f >= 1
 *   drift: the running sum of velocity in BLOCKS of 256 frames.  p[b][i] = v[256 b] + .. + v[256 b + i] sequentially
 *          (np.cumsum of the block); T[b] = p[b][255]; O[b] = T[0] + .. + T[b - 1] sequentially (np.cumsum of the totals);
 *          drift[256 b + i] = O[b] + p[b][i] for b >= 1 and p[0][i] for b = 0.  drift[f] depends on velocity[0 .. f] alone.
 * One thread per (frame, axis) for velocity; one workgroup for drift (thread b sums block b, 65 536 frames a pass).
 *
 * Both: arguments are validated before any HIP call (sizes, mode, the median's limit, null pointers); F = 0 is a no-op. */
int mivit_drift_frames(const double *pos, int N, const int *pair_row, int M, const int *frame_offsets, int F, int mode,
                       int max_pairs, double *stat, void *stream);
int mivit_drift_integrate(const double *stat, const int *n_pairs, int F, int half_window, double *velocity, double *drift,
                          void *stream);

/* Per-range maximum-likelihood diffusion coefficient with its standard error, csrc/likelihood.hip: the exact Gaussian
 * likelihood of the increments of a track whose rows each carry a known localisation variance, under motion blur and with
 * frames that may be missing (Berglund 2010; Michalet & Berglund 2012; Relich et al. 2016; no counterpart in the reference).
 * fp64 without contraction, no LDS, no scratch, no atomics; ONE WAVE per range and lane j = candidate j of the search; a
 * range has NO maximum length (its rows are read from global memory in each of the 8 passes) and its outputs are bitwise the
 * same alone, anywhere in a batch and in every launch.
 *
 * pos [N, 2] fp64 (y, x); var [N, 2] fp64, the variance of each coordinate, or null for zeros; frames [N] int32, or null for
 * consecutive frames (the row index); use [N] bytes (non-zero: the row may be used), or null for all rows; offsets [n + 1]
 * int32, the CSR of the row ranges (tracks, segments, runs; entries are clamped to [0, N]: nothing is read out of bounds
 * whatever they hold).  dt > 0; R in [0, 1/4] the motion-blur coefficient (0: instantaneous exposure, 1/6: the whole frame).
 * A row is USABLE when its flag is set, both coordinates are finite and both variances are finite and >= 0.  The usable rows
 * of a range in order, m of them, have frames f_0 < f_1 < .. (the caller's promise; where it is broken the outputs are
 * defined by the arithmetic below and mean nothing), positions X_k and variances v_k per axis; increments d_k = X_{k+1} - X_k
 * with gaps g_k = f_{k+1} - f_k, k = 0 .. m - 2.  Per candidate D, with c1 = (2 D) dt, cR = R c1, and per axis (y, then x, for
 * every k in ascending order; both axes share Q, P and D):
 *   a_k = (c1 (g_k - 2 R) + v_k) + v_{k+1};   b_{k-1} = cR - v_k
 *   e_0 = a_0, z_0 = d_0;   l_k = b_{k-1} r_{k-1};   e_k = a_k - l_k b_{k-1};   z_k = d_k - l_k z_{k-1};   r_k = 1 / e_k
 *   Q = Q + (z_k z_k) r_k;   P = P e_k, kept as mantissa in [0.5, 1) times 2^pe by frexp after every factor (exact)
 *   cost(D) = -2 log L = ((log(mantissa) + pe log 2) + Q) + 2 (m - 1) log(2 pi)
 * A candidate with some e_k that is not > 0, or whose cost is not below +inf, has cost +inf.
 *
 * The search: D_ref = S / ((4 dt) G) with S = sum_k (dy_k dy_k + dx_k dx_k) and G = sum_k g_k in ascending k.  Bracket
 * [lo, hi] = [-20, 4]; six rounds of: step = (hi - lo) / 63, u_j = lo + j step, D_j = D_ref exp2(u_j) for j = 0 .. 63; j* the
 * least cost, the LOWEST j on a tie; [lo, hi] = [u_max(j* - 1, 0), u_min(j* + 1, 63)].  D = D_{j*} of the last round (the
 * bracket is then 2.4e-8 wide).  status 2 where j* = 0 in every round (the track does not move within its noise): D = 0.
 * status 3 where j* = 63 in every round.  Then c0, c+, c- = cost at D, D e^h, D e^-h with h = 1 / 64 (the factors as fp64
 * constants), loglik = -c0 / 2, and the observed information in ln D, I = ((c+ - c0) + (c- - c0)) / (2 h^2); D_std = D /
 * sqrt(I) where 0 < I < inf, else NaN and status 4 if it was 0.  status 2 has D_std NaN.
 * out, per range: D, D_std, loglik [n] fp64, n_increments [n] int32 = max(m - 1, 0), status [n] int32: 0 fine, 1 fewer than 2
 * increments (D, D_std and loglik NaN), 2, 3, 4 as above.  The only operations that may differ from the numpy restatement
 * (helpers/msd._diffusion_ml_numpy) are log and exp2.  Arguments are validated before any HIP call (sizes, dt, R, null
 * pointers; pos may be null where N = 0); n = 0 is a no-op. */
int mivit_track_diffusion_ml(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                             const int *offsets, int n, double dt, double R, double *D, double *D_std, double *loglik,
                             int *n_increments, int *status, void *stream);

/* Per-range exact log-likelihood of anomalous diffusion, and its maximum over the exponent alpha and the generalised
 * diffusion coefficient D with error bars, csrc/fbm_ml.hip: the Gaussian likelihood of the increments of a track that is
 * a fractional Brownian motion averaged over the camera's exposure, whose rows each carry a known localisation variance and
 * whose frames may be missing (no counterpart in the reference).  fp64 without contraction, no atomics, no scratch.  ONE
 * WORKGROUP (192 threads, 81 320 B of LDS) per range and candidate; a range's outputs are bitwise the same alone, anywhere in
 * a batch and in every launch.  LIMITS: a range may have at most 129 usable rows (ops.FBM_ML_MAX_ROWS) and its usable frames
 * may span at most 1199 (largest - smallest, ops.FBM_ML_MAX_SPAN); a range beyond either gets status 5 and NaN, and nothing
 * is read or written out of bounds whatever the range holds.  The range itself may be of any length.
 *
 * pos, var, frames, use, N, offsets, n, dt: as mivit_track_diffusion_ml, and so is the rule for a USABLE row.  exposure E in
 * [0, 1], the part of a frame, from its start, over which the camera integrates.  The usable rows of a range, m + 1 of
 * them, have frames f_0 < f_1 < .. (the caller's promise), positions X_k, variances v_k per axis; d_k = X_{k+1} - X_k, k = 0
 * .. m - 1.  The structure function at a lag of t >= 0 frames, tau = (double)t:
 *   E = 0:  S(0) = 0, S(t) = pow(tau, alpha)
 *   E > 0:  S(0) = (2 pow(E, alpha)) / a12 with a12 = (alpha + 1) (alpha + 2)
 *           where E > tau / 2 (t = 1 only):  S = ((pow(tau + E, p) + pow(|tau - E|, p)) - 2 pow(tau, p)) / ((E E) a12), p = alpha + 2
 *           else  S = pow(tau, alpha) sum, sum = 1 + t_1 + .. + t_30 added in this order, t_0 = 1,
 *                 t_j = (t_{j-1} (((alpha - 2j + 2) (alpha - 2j + 1)) / ((2j + 1) (2j + 2)))) ((E / tau) (E / tau))
 * Per axis (y, then x; each has its own matrix because each has its own variances) the covariance of the increments, i >= j:
 *   C_ij = (D dt) (((S|f_{i+1} - f_j| + S|f_i - f_{j+1}|) - S|f_{i+1} - f_{j+1}|) - S|f_i - f_j|), then for j = i:
 *   (C_ii + v_i) + v_{i+1}, for j = i - 1: C_ij - v_i.  The per-axis ensemble MSD at a lag t is 2 D dt t^alpha (E = 0), and at
 *   alpha = 1 this is the covariance of mivit_track_diffusion_ml with R = E / 6.
 * The factorisation is left-looking with the increments as row m (C_mj = d_j): for j = 0 .. m - 1, p_j = C_jj - sum_{k<j} L_jk
 * L_jk and, for every i > j, L_ij = (C_ij - sum_{k<j} L_ik L_jk) / sqrt(p_j), each sum subtracted term by term in ascending k;
 * z_j = L_mj.  Q = Q + z_j z_j and P = P p_j (mantissa in [0.5, 1) times 2^pe by frexp after every factor) run over j and over
 * both axes;  cost(alpha, D) = -2 log L = ((log(mantissa) + pe log 2) + Q) + 2 m log(2 pi).  A candidate with some p_j that
 * is not > 0, or whose cost is not below +inf, has cost +inf.
 *
 * mivit_track_fbm_loglik: alpha [n], D [n] fp64 in -> loglik [n] = -cost / 2 (-inf for a rejected candidate), n_increments
 * [n] = max(usable rows - 1, 0), status [n]: 0 fine; 5 over a limit; else 1 no increment; else 6 alpha outside (0, 2) or D
 * negative or not finite; loglik is NaN for 1, 5, 6.
 *
 * mivit_track_fbm_ml: the search.  D_ref = S2 / ((4 dt) (f_m - f_0)), S2 = sum_k (dy_k dy_k + dx_k dx_k) in ascending k.  The
 * bracket starts as alpha in [0.05, 1.95] (helpers/generation.ALPHA_MIN, ALPHA_MAX) and u = log2(D / D_ref) in [-12, 4].
 * 20 rounds of: sa = (ahi - alo) / 7, su = (uhi - ulo) / 7, candidate c = 8 i + j at alpha_i = alo + i sa, D_j = D_ref exp2(ulo +
 * j su); c* the least cost, the LOWEST c on a tie; the next bracket is [max(alpha_i* - 2 sa, 0.05), min(alpha_i* + 2 sa, 1.95)]
 * and [u_j* - 2 su, u_j* + 2 su] (not clamped).  The result is the best candidate of the last round, whose next bracket
 * would be 2.6e-5 wide in alpha and 2.2e-4 in u.  status 2 where j* = 0 in every round (the track does not move within its
 * noise): D = 0, alpha and the bars NaN, loglik the likelihood at D = 0.  status 3 where j* = 7 in every round.  Then the cost
 * c_ab at (alpha + a h, D e^{b h}), a, b in {-1, 0, 1}, h = 1 / 64 (e^h, e^-h as fp64 constants); loglik = -c_00 / 2;
 *   Haa = ((c_+0 - c_00) + (c_-0 - c_00)) 2048, Hdd = ((c_0+ - c_00) + (c_0- - c_00)) 2048, Had = ((c_++ - c_+-) - (c_-+ - c_--)) 512,
 *   det = Haa Hdd - Had Had; alpha_std = sqrt(Hdd / det), D_std = D sqrt(Haa / det), corr = -Had / sqrt(Haa Hdd)
 * where alpha - h >= 0.05, alpha + h <= 1.95, Haa > 0, Hdd > 0 and 0 < det < inf; else the three are NaN and status 4 if it
 * was 0.  out, per range: alpha, alpha_std, D, D_std, corr, loglik [n] fp64, n_increments, status [n] int32: 0 fine; 5 over a
 * limit (NaN); else 1 fewer than 3 increments (NaN); 2, 3, 4 as above.  workspace: at least 640 n bytes, 8-byte aligned; its
 * contents before the call do not matter and mean nothing after it.  The launches (20 x 2 + 2) are queued on the stream
 * without a host synchronisation.  helpers/msd._fbm_ml_numpy restates the search with LAPACK's Cholesky: equal apart from
 * the order of the sums, pow, exp2 and log.  Arguments are validated before any HIP call (sizes, n <= 2^24, dt, exposure,
 * null pointers, the workspace; pos may be null where N = 0); n = 0 is a no-op. */
int mivit_track_fbm_loglik(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                           const int *offsets, int n, double dt, double exposure, const double *alpha, const double *D,
                           double *loglik, int *n_increments, int *status, void *stream);
int mivit_track_fbm_ml(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                       const int *offsets, int n, double dt, double exposure, double *alpha, double *alpha_std, double *D,
                       double *D_std, double *corr, double *loglik, int *n_increments, int *status, void *workspace,
                       size_t workspace_bytes, void *stream);

/* Per-range maximum-likelihood CONFINEMENT radius with error bars, and the exact log-likelihood of confined diffusion at
 * given parameters, csrc/confined_ml.hip: an isotropic Ornstein-Uhlenbeck process (diffusion in a harmonic well) whose rows
 * each carry a known localisation variance and whose frames may be missing (no counterpart in the reference).  The exposure
 * is INSTANTANEOUS: motion blur is not modelled.  fp64 without contraction, no LDS, no scratch, no atomics; ONE WAVE per
 * range, lane 8 i + j = candidate (D_i, s2_j); a range has NO maximum length (its rows are read from global memory in each
 * of the 23 passes) and its outputs are bitwise the same alone, anywhere in a batch and in every launch.
 *
 * pos, var, frames, use, N, offsets, n, dt: as mivit_track_diffusion_ml, and so is the rule for a USABLE row.  The usable rows
 * of a range in order, m of them, have frames f_0 < f_1 < .. (the caller's promise), positions y_k and variances v_k per
 * axis.  Parameters: the diffusion coefficient D and the stationary variance per axis s2; the rate is lam = D / s2 and each
 * axis has a centre c.  Per candidate ldt = (D / s2) dt; pm = 0.5, pe = 1; per axis (y, then x, within every row) the state
 * after row 0 is a = y_0, b = 0, P = v_0 (the filter is conditioned on the first usable row: a diffuse prior on the start;
 * the mean of the state is a + b c), Syy = Syh = Shh = 0.  For every further row k in ascending order, g = f_k - f_{k-1}:
 *   t = ldt (double)g;   om = -expm1(-t);   phi = 1 - om;   q = s2 (-expm1(-(2 t)))          (shared by the axes)
 *   Pm = (phi phi) P + q;   F = Pm + v_k;   r = 1 / F;   am = phi a;   eh = phi b + om;   ey = y_k - am;   K = Pm r
 *   a = am + K ey;   b = eh - K eh;   P = (1 - K) Pm
 *   Syy = Syy + (ey ey) r;   Syh = Syh + (ey eh) r;   Shh = Shh + (eh eh) r
 *   the determinant, shared by the axes: pm = pm F, kept as mantissa in [0.5, 1) times 2^pe by frexp after every factor
 * Centre given:    Q = (Syy - (2 c) Syh) + (c c) Shh per axis.
 * Centre profiled: c = Syh / Shh and Q = Syy - (Syh Syh) / Shh where Shh > 0, else c = NaN and Q = Syy; the standard error of
 *                  the centre is 1 / sqrt(Shh).
 *   cost = -2 log L = ((log(pm) + pe log 2) + (Q_y + Q_x)) + 2 (m - 1) log(2 pi)
 * A candidate with some F that is not > 0, or whose cost is not below +inf, has cost +inf.  As s2 -> inf at a fixed centre
 * this is the likelihood of mivit_track_diffusion_ml at R = 0.
 *
 * mivit_track_confined_loglik: D [n], s2 [n] fp64 in, centre [n, 2] fp64 (y, x) or null to profile it -> loglik [n] = -cost /
 * 2 (-inf for a rejected candidate); NaN for a range with fewer than 2 usable rows and where D or s2 is not positive and
 * finite.  One THREAD per range runs the same device function.
 *
 * mivit_track_confined_ml: the search over (u, w) = (log2 D / D_ref, log2 s2 / S_ref).  D_ref = S / ((4 dt) G) as in
 * mivit_track_diffusion_ml.  S_ref: my = (y_0 + y_1 + ..) / m in ascending order, mx alike, then S_ref = (sum_k ((y_k - my)
 * (y_k - my) + (x_k - mx) (x_k - mx))) / (2 m) in ascending k: half the summed variance of the usable positions.  Brackets u
 * in [-12, 4], w in [-6, 18].  20 rounds of: su = (uhi - ulo) / 7, sw = (whi - wlo) / 7, candidate 8 i + j at D_i = D_ref
 * exp2(ulo + i su), s2_j = S_ref exp2(wlo + j sw) with the centre profiled; the least cost, the LOWEST candidate on a tie;
 * ub = ulo + i* su, wb = wlo + j* sw; the next brackets are [ub - 2 su, ub + 2 su] and [wb - 2 sw, wb + 2 sw] (not clamped).
 * The result is the best candidate of the last round, D = D_ref exp2(ub), s2 = S_ref exp2(wb), whose next brackets would
 * be 2.2e-4 wide in u and 3.3e-4 in w.  lam = D / s2.  status, the first that applies of: 2 where wb >= 18 (s2 left its first
 * bracket upwards: the well is wider than the search can see, the track is not confined; this holds in particular where
 * j* = 7 in every round); 3 where lam dt > 4 (the particle relaxes within a frame); 5 where i* = 0 in every round, or i* = 7
 * in every round, or j* = 0 in every round; else 0.  Then the cost c_ab at (D e^{a h}, s2 e^{b h}), a, b in {-1, 0, 1}, h = 1 /
 * 64 (e^h, e^-h as fp64 constants; lane 3 (a + 1) + (b + 1), the other lanes repeat lane 0); loglik = -c_00 / 2; the centre and
 * Shh come from the lane of c_00;
 *   Hdd = ((c_+0 - c_00) + (c_-0 - c_00)) 2048, Hss = ((c_0+ - c_00) + (c_0- - c_00)) 2048, Hds = ((c_++ - c_+-) - (c_-+ - c_--)) 512,
 *   det = Hdd Hss - Hds Hds;  pd = Hdd > 0 and Hss > 0 and 0 < det < inf
 * status 4 where c_00 is not below +inf (no candidate was accepted; whatever the status was), and where pd fails and the
 * status was 0.  Where pd holds and the status is 0 or 5: D_std = D sqrt(Hss / det), radius_std = (radius / 2) sqrt(Hdd / det),
 * corr = -Hds / sqrt(Hdd Hss), lambda_std = lam sqrt(vl) with vl = ((Hss + Hdd) + 2 Hds) / det (the delta method: var ln lam =
 * var ln D + var ln s2 - 2 cov) where vl >= 0; else they are NaN, but status 3 has radius_std = (radius / 2) / sqrt(Hss) where
 * 0 < Hss < inf (D is not identified; s2 at the D found).
 * out, per range: D, D_std, radius = sqrt(2 s2) (the RMS distance from the centre in 2-D; +inf for status 2), radius_std,
 * lambda = lam (0 for status 2), lambda_std, corr, loglik [n] fp64; centre, centre_std [n, 2] fp64 (y, x; NaN for status 2,
 * centre_std = 1 / sqrt(Shh) where Shh > 0 and NaN for status 4); n_increments [n] int32 = max(m - 1, 0); status [n] int32: 0
 * fine, 1 fewer than 4 increments (every fp64 output NaN), 2 .. 5 as above.  The only operations that may differ from the
 * numpy restatement (helpers/msd._confined_ml_numpy) are expm1, exp2 and log.  Arguments are validated before any HIP call
 * (sizes, dt, null pointers; pos may be null where N = 0; var, frames, use and the centre of the log-likelihood may be null);
 * n = 0 is a no-op. */
int mivit_track_confined_ml(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                            const int *offsets, int n, double dt, double *D, double *D_std, double *radius, double *radius_std,
                            double *lambda, double *lambda_std, double *corr, double *centre, double *centre_std, double *loglik,
                            int *n_increments, int *status, void *stream);
int mivit_track_confined_loglik(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                                const int *offsets, int n, double dt, const double *D, const double *s2, const double *centre,
                                double *loglik, void *stream);

/* Per-range maximum-likelihood VELOCITY and diffusion coefficient of directed motion with error bars, and the exact
 * log-likelihood of directed motion at given parameters, csrc/directed_ml.hip: the model of mivit_track_diffusion_ml with a
 * mean, diffusion plus a constant velocity u per axis (no counterpart in the reference).  The increments keep their
 * tridiagonal covariance; their mean is u m_k with m_k = g_k dt (an exposure average shifts every row of a track of constant
 * velocity alike, so blur leaves the mean alone).  fp64 without contraction, no LDS, no scratch, no atomics; ONE WAVE per
 * range and lane j = candidate j of the search over D; a range has NO maximum length (its rows are read from global memory
 * in each of the 9 passes) and its outputs are bitwise the same alone, anywhere in a batch and in every launch.
 *
 * pos, var, frames, use, N, offsets, n, dt, R: as mivit_track_diffusion_ml, and so are the rule for a USABLE row and the names
 * X_k, v_k, f_k, d_k, g_k of the m usable rows and their m - 1 increments.
 * The cost at D ABOUT A VELOCITY (wy, wx): per increment g = (double)g_k, mk = g dt, and per axis (y, then x, for every k in
 * ascending order) dd_k = d_k - w mk; c1 = (2 D) dt, cR = R c1; a_k, b_{k-1}, l_k, e_k, r_k as in mivit_track_diffusion_ml, and
 *   z_0 = dd_0, t_0 = mk;   z_k = dd_k - l_k z_{k-1};   t_k = mk - l_k t_{k-1}      (two residuals under one multiplier and pivot)
 *   A = A + (z_k z_k) r_k;   B = B + (z_k t_k) r_k;   C = C + (t_k t_k) r_k         (per axis)
 *   P = P e_k, shared by the axes, kept as mantissa in [0.5, 1) times 2^pe by frexp after every factor (exact)
 * Velocity given (it is w):  Q = A_y + A_x.
 * Velocity profiled:         Q = (A_y - (B_y B_y) / C_y) + (A_x - (B_x B_x) / C_x).
 * Either way the velocity of the fit is u = w + B / C per axis and its standard error at this D is 1 / sqrt(C): for Gaussian
 * data the mean and the covariance parameters share no Fisher information.
 *   cost = -2 log L = ((log(mantissa) + pe log 2) + Q) + 2 (m - 1) log(2 pi)
 * A candidate with some e_k that is not > 0, with a C that is not > 0 or not finite, or whose cost is not below +inf, has cost
 * +inf.  The profile does not depend on w in exact arithmetic (A - B B / C is invariant under d -> d - w m, and u with it);
 * in fp64 a w near the answer keeps A, B and C of the size of the noise however fast the track is, so nothing cancels.
 *
 * mivit_track_directed_ml.  Pass 0: m, G = sum_k g_k, and the UNWEIGHTED velocity u0 = (X_{m-1} - X_0) / ((double)G dt) per
 * axis.  Pass 1: D_ref = S / ((4 dt) G) with S = sum_k (dd_k,y dd_k,y + dd_k,x dd_k,x) in ascending k and dd taken about u0: the
 * reference scale holds no velocity, so a fast, quiet track keeps its optimum inside the bracket and a velocity added to a
 * track changes D by rounding alone.  Then the search of mivit_track_diffusion_ml (bracket [-20, 4], six rounds of 64
 * candidates, D_j = D_ref exp2(u_j), the LOWEST j on a tie, statuses 2 and 3) on the profiled cost about w = u0, the three
 * costs at D, D e^h, D e^-h (lanes 0, 1, 2), loglik = -c0 / 2, D_std = D / sqrt(I) and status 4 as there.  Lane 0 writes v = u0
 * + B / C and v_std = 1 / sqrt(C) of its own sums at D, per axis, where c0 is below +inf, else NaN (status 2 with zero
 * variances: the likelihood at D = 0 does not exist).  This is plain maximum likelihood, not REML: D is low by about one part
 * in m - 1.
 * out, per range: D, D_std [n], v, v_std [n, 2] (y, x) in pixels per unit of dt, loglik [n] fp64, n_increments [n] int32 = max(m -
 * 1, 0), status [n] int32: 0 fine, 1 fewer than 2 increments (every fp64 output NaN), 2 the minimum at the lower end (D = 0,
 * D_std NaN), 3 at the upper end, 4 the curvature is not positive (D_std NaN).
 *
 * mivit_track_directed_loglik: D [n] fp64 in; v [n, 2] fp64 (y, x) in, or null to profile the velocity (w is then u0 of pass
 * 0) -> loglik [n] = -cost / 2 (-inf for a rejected candidate); NaN for a range with fewer than 2 usable rows, where D is
 * negative or not finite and where a given velocity is not finite.  v_hat, v_hat_std [n, 2] fp64 or null: where given, the
 * velocity u of the fit and 1 / sqrt(C), NaN where loglik is not finite.  One THREAD per range runs the same device function.
 * With v = 0 the cost is that of mivit_track_diffusion_ml at D but for the order in which Q is added up.
 * The only operations that may differ from the numpy restatements (helpers/msd._directed_ml_numpy, _directed_loglik_numpy)
 * are log and exp2.  Arguments are validated before any HIP call (sizes, dt, R, null pointers; pos may be null where N = 0;
 * var, frames, use, v, v_hat and v_hat_std may be null); n = 0 is a no-op. */
int mivit_track_directed_ml(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                            const int *offsets, int n, double dt, double R, double *D, double *D_std, double *v, double *v_std,
                            double *loglik, int *n_increments, int *status, void *stream);
int mivit_track_directed_loglik(const double *pos, const double *var, const int *frames, const unsigned char *use, int N,
                                const int *offsets, int n, double dt, double R, const double *D, const double *v, double *loglik,
                                double *v_hat, double *v_hat_std, void *stream);

/* Run-and-pause transport, csrc/segment.hip: tracks whose VELOCITY changes (motor-driven cargo that runs, pauses and runs
 * again; no counterpart in the reference).  Both in fp64 without contraction, no atomics, a track's / stretch's result bitwise
 * the same alone, in any batch and in every launch.
 *
 * mivit_segment_transport: the optimal partition of every track into stretches that are each diffusive (class 0: zero-mean
 * increments of one variance) or directed (class 1: one variance about a constant velocity), one wave per track.  pos, offsets
 * and max_len as mivit_segment_tracks takes them, max_len <= 4096 (cs2, csy, csx, F and prev live in LDS, 36 B a row: 147 456 B
 * at the limit; classes = 2 runs the kernel of mivit_segment_tracks, 20 B a row; a larger value is an error, never a launch).
 * A track of L rows has Linc = L - 1 increments (dy_k, dx_k) between rows k and k + 1, and three prefix sums, each summed in
 * ascending k by one lane (np.cumsum bit for bit):
 *   cs2[j] = sum_{k<j} (dy_k dy_k + dx_k dx_k);   csy[j] = sum_{k<j} dy_k;   csx[j] = sum_{k<j} dx_k
 * With n = j - i, SS = cs2[j] - cs2[i], Sy = csy[j] - csy[i], Sx = csx[j] - csx[i], lg = log(Linc), beta = penalty * lg and
 * gamma = velocity_penalty * lg:
 *   C0(i, j) = (2 n) * log(max(SS / (2 n), min_var))                                  the cost of mivit_segment_tracks
 *   C1(i, j) = (2 n) * log(max((SS - (Sy Sy + Sx Sx) / n) / (2 n), min_var)) + gamma  the velocity profiled out per axis
 *   classes 0 (both):      C = C1 if C1 < C0 else C0, class 1 only where C1 is strictly lower (a tie and a NaN are diffusive)
 *   classes 1 (directed):  C = C1, class 1;      classes 2 (diffusive): C = C0, class 0
 *   F(0) = -beta;  F(j) = min over i in {0} and [min_len, j - min_len] of (F(i) + C(i, j)) + beta,   j = min_len .. Linc
 * max keeps a NaN and lifts a residual that rounding made negative.  prev[j] is the LOWEST i among equal minima, kept as 2 i +
 * the class of the stretch (i, j); backtracking prev from Linc gives the changepoints and the class of every stretch, which the
 * wave writes to the stretch's rows as it walks.  Linc < 2 min_len leaves only i = 0; 1 <= Linc < min_len has no step and gets
 * F(Linc) = (F(0) + C(0, Linc)) + beta with its class by the same rule.  Where every candidate is NaN, prev[j] = 0 and the
 * class is 0.  The sums are not centred: SS - S^2 / n cancels for a fast track, but by less than the rounding of F at any
 * speed a linker can follow.
 * out: seg_start [N] int32, 1 on the first row of every stretch as mivit_segment_tracks writes it; seg_class [N] int32, the
 * class of the stretch each row belongs to (a one-row track: 0); cost [n_tracks] fp64 = F(Linc), NaN where Linc < 1.  An empty
 * track writes nothing.  With classes = 2 seg_start and cost are those of mivit_segment_tracks bit for bit.  The only
 * operation that may differ from the numpy restatement (helpers/msd._transport_numpy) is log.  min_len >= 2, penalty >= 0,
 * velocity_penalty >= 0, min_var > 0 and finite.  Arguments are validated before any HIP call; n_tracks = 0 is a no-op.
 *
 * mivit_transport_stats: one row of estimates per stretch about the stretch's own velocity, one thread per stretch.
 * seg_offsets, seg_track_end, the rows and the bridging increment as mivit_segment_stats; n the number of increments.  Sums
 * in ascending index, starting from 0.0:
 *   pass 1:  my = (sum_k dy_k) / n,  mx = (sum_k dx_k) / n;   velocity[s] = (my / dt, mx / dt)
 *   pass 2:  ey_k = dy_k - my,  ex_k = dx_k - mx
 *            S2 = sum_k (ey_k ey_k + ex_k ex_k);   S11 = sum_k (ey_k ey_{k+1} + ex_k ex_{k+1}) over the n - 1 neighbouring pairs
 *   D_res  = S2 / ((4 n) dt)
 *   D_cve  = D_res + S11 / ((2 (n - 1)) dt)                             Vestergaard et al. 2014 about the velocity:
 *   sigma2 = (R S2) / (2 n) + ((2 R - 1) S11) / (2 (n - 1))             localisation noise and blur cancel as above
 * NaN where n < 1 (velocity, D_res) and where n < 2 (D_cve, sigma2); velocity [n_seg, 2], n_increments [n_seg] int32.  No
 * log: bitwise the numpy restatement (helpers/msd._transport_stats_numpy).  Rows are clamped to [0, N - 1].  dt > 0, R in [0,
 * 1/4].  n_seg = 0 is a no-op. */
int mivit_segment_transport(const double *pos, int N, const int *offsets, int n_tracks, int max_len, int min_len, double penalty,
                            double velocity_penalty, double min_var, int classes, int *seg_start, int *seg_class, double *cost,
                            void *stream);
int mivit_transport_stats(const double *pos, int N, const int *seg_offsets, const int *seg_track_end, int n_seg, double dt,
                          double R, double *velocity, double *d_res, double *d_cve, double *sigma2, int *n_increments,
                          void *stream);

/* LayerNorm-1 backward + out-projection backward in one pass (autograd of x1 = LN1(x + out_proj(ctx)), models.py:57,100-102,
 * between the feed-forward block's input gradient and the attention core), csrc/fused_bwd.hip:
 * in : dy = dL/dx1 [M,E] bf16, n1 / rstd1 (LN1's normalised output, 1/std), gamma1, ctx [M,E] (out_proj's input), Wo bf16 [E,E];
 * out: dz1 = dL/d(x + out_proj(ctx)) [M,E] bf16 (also the residual branch's gradient), dctx = dz1 Wo [M,E] bf16,
 *      dWo [E,E], dbo [E], dgamma1 [E], dbeta1 [E] fp32 (overwritten).  Deterministic. */
size_t mivit_attn_out_bwd_workspace_bytes(int M);
int mivit_attn_out_bwd(const void *dy, const void *n1, const float *rstd1, const float *gamma1, const void *ctx,
                       const void *Wo_bf16, int M, void *dz1, void *dctx, float *dWo, float *dbo, float *dgamma1,
                       float *dbeta1, void *workspace, size_t workspace_bytes, void *stream);

/* q|k|v projection backward in one pass over dqkv (autograd of qkv = x Wqkv^T + bqkv, helpers/models.py:42-44, joined by the
 * residual branch's gradient, :100-102), csrc/fused_bwd.hip:
 * in : dqkv [M,3E] bf16 (from mivit_attention_bwd), x [M,E] bf16 (the projection's input rows), Wqkv bf16 [3E,E], res [M,E] bf16;
 * out: dx = dqkv Wqkv + res [M,E] bf16;  dW = dqkv^T x [3E,E], db = column sums of dqkv [3E], fp32 (overwritten).  Deterministic.
 * E = 128 (and E = 64 as ..._w64). */
size_t mivit_qkv_bwd_workspace_bytes(int M);
int mivit_qkv_bwd(const void *dqkv, const void *x, const void *Wqkv_bf16, const void *res, int M, void *dx, float *dW, float *db,
                  void *workspace, size_t workspace_bytes, void *stream);
/* The same with the projection's input given as x = fix_gamma * n + fix_beta, where `x` above holds n (a LayerNorm's normalised
 * output, fix_gamma / fix_beta [E] fp32 its affine): dW = dqkv^T (fix_gamma * n + fix_beta) = (dqkv^T n) diag(fix_gamma) +
 * db (x) fix_beta, applied to each workgroup's partial sums (the engine's path for every layer after the first); dx and db as
 * above.  fix_gamma = fix_beta = NULL is mivit_qkv_bwd. */
int mivit_qkv_bwd_affine(const void *dqkv, const void *x, const void *Wqkv_bf16, const void *res, int M, void *dx, float *dW,
                         float *db, const float *fix_gamma, const float *fix_beta, void *workspace, size_t workspace_bytes,
                         void *stream);
size_t mivit_qkv_bwd_workspace_bytes_w64(int M);
int mivit_qkv_bwd_w64(const void *dqkv, const void *x, const void *Wqkv_bf16, const void *res, int M, void *dx, float *dW, float *db,
                      void *workspace, size_t workspace_bytes, void *stream);
int mivit_qkv_bwd_affine_w64(const void *dqkv, const void *x, const void *Wqkv_bf16, const void *res, int M, void *dx, float *dW,
                             float *db, const float *fix_gamma, const float *fix_beta, void *workspace, size_t workspace_bytes,
                             void *stream);

/* The same five operators for the reference's shipped layer width: E = 64, F = 128, 4 heads of 16
 * (Experiments/Framerate/trainSettingsFramerate.py:42-47, Experiments/ImagesFeatures/...:112-188): csrc/fused_fwd.hip and
 * csrc/fused_bwd.hip compiled a second time with -DMIVIT_WIDTH64.  Same arguments, layouts and optional outputs. */
int mivit_fused_layer_supported_w64(int dtype, int embed_dim, int hidden_dim, int num_heads, int tokens);
int mivit_attn_block_fwd_w64(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv_bf16,
                             const float *bqkv, const void *Wo_bf16, const float *bo, const float *gamma_out,
                             const float *beta_out, int B, int S, void *ctx, void *n_out, float *rstd, void *x_out,
                             void *z_out, float *mean, void *qkv_out, void *stream);
int mivit_mlp_block_fwd_w64(const void *n_in, const float *gamma_in, const float *beta_in, const void *W1_bf16,
                            const float *b1, const void *W2_bf16, const float *b2, const float *gamma_out,
                            const float *beta_out, int M, int act, void *n_out, float *rstd, void *x_out, void *z_out,
                            float *mean, void *h_out, void *u_out, void *stream);
size_t mivit_mlp_block_bwd_workspace_bytes_w64(int M);
int mivit_mlp_block_bwd_w64(const void *dy, const void *n2, const float *rstd2, const float *gamma2, const void *n1,
                            const float *gamma1, const float *beta1, const void *W1_bf16, const float *b1, const void *W2_bf16,
                            int M, int act, void *dx1, float *dW1, float *db1, float *dW2, float *db2, float *dgamma2,
                            float *dbeta2, void *workspace, size_t workspace_bytes, void *stream);
size_t mivit_attn_out_bwd_workspace_bytes_w64(int M);
int mivit_attn_out_bwd_w64(const void *dy, const void *n1, const float *rstd1, const float *gamma1, const void *ctx,
                           const void *Wo_bf16, int M, void *dz1, void *dctx, float *dWo, float *dbo, float *dgamma1,
                           float *dbeta1, void *workspace, size_t workspace_bytes, void *stream);

/* The five operators in IEEE half (fp16 models: the engine's fp16 layer path): csrc/fused_fwd.hip and csrc/fused_bwd.hip
 * compiled with -DMIVIT_ELEM_F16, at width 128 (..._f16) and width 64 (..._w64_f16).  Same arguments and layouts as above with
 * every 16-bit tensor (activations, gradients and weight copies) in fp16; biases, LayerNorm vectors, rstd / mean and the
 * parameter gradients stay fp32.  mivit_mlp_block_bwd_set_waves_f16 is the fp16 width-128 build's kernel switch. */
int mivit_fused_layer_supported_f16(int dtype, int embed_dim, int hidden_dim, int num_heads, int tokens);
int mivit_attn_block_fwd_f16(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv,
                             const float *bqkv, const void *Wo, const float *bo, const float *gamma_out,
                             const float *beta_out, int B, int S, void *ctx, void *n_out, float *rstd, void *x_out,
                             void *z_out, float *mean, void *qkv_out, void *stream);
int mivit_mlp_block_fwd_f16(const void *n_in, const float *gamma_in, const float *beta_in, const void *W1,
                            const float *b1, const void *W2, const float *b2, const float *gamma_out,
                            const float *beta_out, int M, int act, void *n_out, float *rstd, void *x_out, void *z_out,
                            float *mean, void *h_out, void *u_out, void *stream);
size_t mivit_mlp_block_bwd_workspace_bytes_f16(int M);
int mivit_mlp_block_bwd_f16(const void *dy, const void *n2, const float *rstd2, const float *gamma2, const void *n1,
                            const float *gamma1, const float *beta1, const void *W1, const float *b1, const void *W2,
                            int M, int act, void *dx1, float *dW1, float *db1, float *dW2, float *db2, float *dgamma2,
                            float *dbeta2, void *workspace, size_t workspace_bytes, void *stream);
size_t mivit_attn_out_bwd_workspace_bytes_f16(int M);
int mivit_attn_out_bwd_f16(const void *dy, const void *n1, const float *rstd1, const float *gamma1, const void *ctx,
                           const void *Wo, int M, void *dz1, void *dctx, float *dWo, float *dbo, float *dgamma1,
                           float *dbeta1, void *workspace, size_t workspace_bytes, void *stream);
size_t mivit_qkv_bwd_workspace_bytes_f16(int M);
int mivit_qkv_bwd_f16(const void *dqkv, const void *x, const void *Wqkv, const void *res, int M, void *dx, float *dW, float *db,
                      void *workspace, size_t workspace_bytes, void *stream);
int mivit_qkv_bwd_affine_f16(const void *dqkv, const void *x, const void *Wqkv, const void *res, int M, void *dx, float *dW,
                             float *db, const float *fix_gamma, const float *fix_beta, void *workspace, size_t workspace_bytes,
                             void *stream);
int mivit_mlp_block_bwd_set_waves_f16(int waves);
int mivit_fused_layer_supported_w64_f16(int dtype, int embed_dim, int hidden_dim, int num_heads, int tokens);
int mivit_attn_block_fwd_w64_f16(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv,
                                 const float *bqkv, const void *Wo, const float *bo, const float *gamma_out,
                                 const float *beta_out, int B, int S, void *ctx, void *n_out, float *rstd, void *x_out,
                                 void *z_out, float *mean, void *qkv_out, void *stream);
int mivit_mlp_block_fwd_w64_f16(const void *n_in, const float *gamma_in, const float *beta_in, const void *W1,
                                const float *b1, const void *W2, const float *b2, const float *gamma_out,
                                const float *beta_out, int M, int act, void *n_out, float *rstd, void *x_out, void *z_out,
                                float *mean, void *h_out, void *u_out, void *stream);
size_t mivit_mlp_block_bwd_workspace_bytes_w64_f16(int M);
int mivit_mlp_block_bwd_w64_f16(const void *dy, const void *n2, const float *rstd2, const float *gamma2, const void *n1,
                                const float *gamma1, const float *beta1, const void *W1, const float *b1, const void *W2,
                                int M, int act, void *dx1, float *dW1, float *db1, float *dW2, float *db2, float *dgamma2,
                                float *dbeta2, void *workspace, size_t workspace_bytes, void *stream);
size_t mivit_attn_out_bwd_workspace_bytes_w64_f16(int M);
int mivit_attn_out_bwd_w64_f16(const void *dy, const void *n1, const float *rstd1, const float *gamma1, const void *ctx,
                               const void *Wo, int M, void *dz1, void *dctx, float *dWo, float *dbo, float *dgamma1,
                               float *dbeta1, void *workspace, size_t workspace_bytes, void *stream);
size_t mivit_qkv_bwd_workspace_bytes_w64_f16(int M);
int mivit_qkv_bwd_w64_f16(const void *dqkv, const void *x, const void *Wqkv, const void *res, int M, void *dx, float *dW, float *db,
                          void *workspace, size_t workspace_bytes, void *stream);
int mivit_qkv_bwd_affine_w64_f16(const void *dqkv, const void *x, const void *Wqkv, const void *res, int M, void *dx, float *dW,
                                 float *db, const float *fix_gamma, const float *fix_beta, void *workspace, size_t workspace_bytes,
                                 void *stream);

/* The last encoder layer under the regression-token readout (csrc/engine.hip, mivit_set_readout_rows(1)): the head reads row 0
 * of every S-token sequence, so in that layer's backward d(x1), d(z1), d(ctx) and dq are exact zeros in every other row.  Two
 * variants of the operators above that neither compute, read nor write what is zero or never read; what they do produce is
 * bitwise what the full operator produces from the same buffers.  Same arguments, layouts and workspaces unless stated.
 *   mivit_attn_block_fwd_q1  : k and v (and their rows of qkv_out) for every row; the query side -- q, attention, out-projection,
 *       residual, LayerNorm -- for the first min(S, 16) rows of a sequence only.  Rows behind them: q, ctx, rstd (x_out, z_out,
 *       mean) are NOT written; n_out is written as zeros when qkv_out is given (a backward follows, and mivit_mlp_block_bwd
 *       reads every row of it) and not written otherwise.  S <= 16: mivit_attn_block_fwd.
 *   mivit_attn_out_bwd_rows  : dy is zero outside the rows r % S == 0 by contract.  Only those rows of dy / n1 / rstd1 / ctx are
 *       read and only those rows of dctx are written; dz1 is written in every row (zeros in the others: mivit_qkv_bwd reads
 *       them all); dWo, dbo, dgamma1, dbeta1 sum the same terms in the same order.
 * Suffixes as above: _w64 (E = 64), _f16, _w64_f16. */
int mivit_attn_block_fwd_q1(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv_bf16,
        const float *bqkv, const void *Wo_bf16, const float *bo, const float *gamma_out, const float *beta_out, int B, int S,
        void *ctx, void *n_out, float *rstd, void *x_out, void *z_out, float *mean, void *qkv_out, void *stream);
int mivit_attn_out_bwd_rows(const void *dy, const void *n1, const float *rstd1, const float *gamma1, const void *ctx,
        const void *Wo_bf16, int M, int S, void *dz1, void *dctx, float *dWo, float *dbo, float *dgamma1, float *dbeta1,
        void *workspace, size_t workspace_bytes, void *stream);
int mivit_attn_block_fwd_q1_w64(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv_bf16,
        const float *bqkv, const void *Wo_bf16, const float *bo, const float *gamma_out, const float *beta_out, int B, int S,
        void *ctx, void *n_out, float *rstd, void *x_out, void *z_out, float *mean, void *qkv_out, void *stream);
int mivit_attn_out_bwd_rows_w64(const void *dy, const void *n1, const float *rstd1, const float *gamma1, const void *ctx,
        const void *Wo_bf16, int M, int S, void *dz1, void *dctx, float *dWo, float *dbo, float *dgamma1, float *dbeta1,
        void *workspace, size_t workspace_bytes, void *stream);
int mivit_attn_block_fwd_q1_f16(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv,
        const float *bqkv, const void *Wo, const float *bo, const float *gamma_out, const float *beta_out, int B, int S,
        void *ctx, void *n_out, float *rstd, void *x_out, void *z_out, float *mean, void *qkv_out, void *stream);
int mivit_attn_out_bwd_rows_f16(const void *dy, const void *n1, const float *rstd1, const float *gamma1, const void *ctx,
        const void *Wo, int M, int S, void *dz1, void *dctx, float *dWo, float *dbo, float *dgamma1, float *dbeta1,
        void *workspace, size_t workspace_bytes, void *stream);
int mivit_attn_block_fwd_q1_w64_f16(const void *n_in, const float *gamma_in, const float *beta_in, const void *Wqkv,
        const float *bqkv, const void *Wo, const float *bo, const float *gamma_out, const float *beta_out, int B, int S,
        void *ctx, void *n_out, float *rstd, void *x_out, void *z_out, float *mean, void *qkv_out, void *stream);
int mivit_attn_out_bwd_rows_w64_f16(const void *dy, const void *n1, const float *rstd1, const float *gamma1, const void *ctx,
        const void *Wo, int M, int S, void *dz1, void *dctx, float *dWo, float *dbo, float *dgamma1, float *dbeta1,
        void *workspace, size_t workspace_bytes, void *stream);

/* DeepResNetEmbedding in inference mode (helpers/models.py:230-257; ResidualBlock :202-228): conv3x3(1->32)+BN+ReLU,
 * ResidualBlock(32->64), ResidualBlock(64->128), global average pool, Linear(128->E), fused in one kernel that keeps F
 * whole frames in LDS.  Eval-mode BatchNorm is folded by the caller: conv weights are pre-scaled by
 * gamma/sqrt(running_var+eps) and laid out [c_out][tap][c_in] (tap = 3*ky+kx) in the compute dtype (fp32 or bf16);
 * the biases are the folded shifts (b12/b22 = main-path shift + skip-path shift), fp32.  w0 [32][9], wfc [E][128] fp32.
 * x [N,P,P] fp32 frames, tokens [N,E] fp32.  Returns 3 if the frame side does not fit
 * (mivit_deepresnet_eval_supported tells beforehand). */
int mivit_deepresnet_eval_supported(int dtype, int patch_size);
int mivit_deepresnet_eval_fwd(int dtype, const float *x, int N, int P, int E, const float *w0, const float *b0,
                              const void *w11, const void *w12, const void *w1s, const void *w21, const void *w22,
                              const void *w2s, const float *b11, const float *b12, const float *b21, const float *b22,
                              const float *wfc, const float *bfc, float *tokens, void *stream);

/* DeepResNetEmbedding in TRAINING mode (batch-statistics BatchNorm2d, helpers/models.py:202-257), forward + backward.
 * Parameters are passed in the reference's own layouts (Conv2d weight [c_out, c_in, kh, kw] fp32, BatchNorm vectors),
 * in the order: 0 initial_conv/bn1, 1 res_block1.conv1/bn1, 2 res_block1.conv2/bn2, 3 res_block1.skip.0/.1,
 * 4 res_block2.conv1/bn1, 5 res_block2.conv2/bn2, 6 res_block2.skip.0/.1.
 * train_fwd: x [N,P,P] fp32 frames -> tokens [N,E] fp32; updates running_mean / running_var in place
 * (running = (1-momentum)*running + momentum*batch, unbiased variance; pass null to skip) and leaves the raw
 * convolution outputs + statistics in `workspace`, which train_bwd of the same step reads (same dtype, N, P, E).
 * train_bwd: dtokens [N,E] fp32 -> every parameter gradient (fp32, reference layouts, overwritten).  There is no
 * gradient w.r.t. x (frames are data).  Activations are stored in the compute dtype (fp32 or bf16), statistics,
 * pooling and the final Linear in fp32.  Returns 3 when the frame side does not fit (ask *_supported first). */
typedef struct { const float *weight, *gamma, *beta; float *running_mean, *running_var; } mivit_conv_bn;
typedef struct { mivit_conv_bn conv[7]; const float *fc_weight, *fc_bias; } mivit_deepresnet_params;
typedef struct { float *weight, *gamma, *beta; } mivit_conv_bn_grad;
typedef struct { mivit_conv_bn_grad conv[7]; float *fc_weight, *fc_bias; } mivit_deepresnet_grads;
int mivit_deepresnet_train_supported(int dtype, int patch_size);
size_t mivit_deepresnet_train_workspace_bytes(int dtype, int N, int P, int E);
int mivit_deepresnet_train_fwd(int dtype, const mivit_deepresnet_params *params, const float *x, int N, int P, int E,
                               float momentum, float eps, float *tokens, void *workspace, size_t workspace_bytes,
                               void *stream);
/* Inference with the layer-by-layer kernels (any frame side): BatchNorm uses running_mean / running_var (required,
 * not modified).  Workspace as for train_fwd. */
int mivit_deepresnet_infer(int dtype, const mivit_deepresnet_params *params, const float *x, int N, int P, int E,
                           float eps, float *tokens, void *workspace, size_t workspace_bytes, void *stream);
int mivit_deepresnet_train_bwd(int dtype, const mivit_deepresnet_params *params, const float *x, const float *dtokens,
                               int N, int P, int E, float eps, const mivit_deepresnet_grads *grads, void *workspace,
                               size_t workspace_bytes, void *stream);

/* Introspection (tests, diagnostics): byte offsets of the training workspace regions -- [0..6] raw convolution outputs
 * y0..y6 ([N*P*P, c_out] in the compute dtype), [7] forward BatchNorm tables (7 x [mean|rstd|scale|shift] x 128 fp32),
 * [8] gradient tables (7 x [k|c0|c1] x 128), [9] pooled [N,128] fp32, [10] dpooled, [11] partial sums, [12..14] the three
 * gradient buffers, [15] total bytes. */
int mivit_deepresnet_train_workspace_layout(int dtype, int N, int P, int E, size_t *offsets /* [16] */);

/* Synchronised BatchNorm for data-parallel training of the DeepResNet embedding (the reference trains on
 * one device, so its BatchNorm2d at helpers/models.py:206-225,233 always sees the whole minibatch -- this keeps that
 * true across ranks).  train_fwd / train_bwd cut into MIVIT_DEEPRESNET_STAGES stages each; call stage 0..5 in order.
 * Every stage leaves this rank's BatchNorm sums in `stats` ([2][3][128] fp64 on the device); between two stages the
 * caller all-reduces (sum) the whole buffer in the forward pass and only its first [3][128] in the backward pass (the
 * second half keeps the local sums that d gamma / d beta are made from, exactly as torch.nn.SyncBatchNorm does), then
 * calls the next stage; *global_count (fp64 on the device, read by the kernels: no host synchronisation) = (frames over
 * all ranks) * P * P, i.e. the all-reduced local N*P*P.  Not replayed as hipGraphs. */
#define MIVIT_DEEPRESNET_STAGES 6
#define MIVIT_DEEPRESNET_STATS_DOUBLES (2 * 3 * 128)
int mivit_deepresnet_train_fwd_stage(int dtype, const mivit_deepresnet_params *params, const float *x, int N, int P, int E,
                                     float momentum, float eps, float *tokens, void *workspace, size_t workspace_bytes,
                                     int stage, const double *global_count, double *stats, void *stream);
int mivit_deepresnet_train_bwd_stage(int dtype, const mivit_deepresnet_params *params, const float *x, const float *dtokens,
                                     int N, int P, int E, float eps, const mivit_deepresnet_grads *grads, void *workspace,
                                     size_t workspace_bytes, int stage, const double *global_count, double *stats, void *stream);

/* Weight gradient of narrow layers (64-wide models), bf16: dW [N,K] = dy^T x for (N, K) in {(64,64), (128,64),
 * (192,64), (64,128)}, M >= 256; the whole gradient block lives in each wave's accumulators, deterministic reduction. */
size_t mivit_wgrad_small_workspace_bytes(int M, int N, int K);
int mivit_wgrad_small(const void *dy, int64_t lddy, const void *x, int64_t ldx, int M, int N, int K, float *dW,
                      float *db /* optional: column sums of dy */, void *workspace, size_t workspace_bytes, void *stream);

/* Row LayerNorm over E, eps 1e-5, biased variance, affine (nn.LayerNorm: models.py:88-89,134,301).
 * Row r of the output goes to row  (r / rows_per_seq) * out_seq_stride + r % rows_per_seq + out_row_off  when
 * rows_per_seq > 0 (token assembly behind the regression token, models.py:347), else to row r.
 * `pos` (optional, fp32 [out_seq_stride, E]) is added after the affine (models.py:137-138).  It is indexed by the position
 * in the OUTPUT sequence, offset included: row r gets pos[(output row) % out_seq_stride], so with out_row_off = 1 the first
 * token of a sequence gets pos[1] and pos[0] (the regression token's) is never read.  With rows_per_seq == 0 there is no
 * sequence structure and every row gets pos[0].
 * mean/rstd (fp32 [M], optional) are saved for backward, indexed by the input row r (never mapped).
 * ldz/ldy in elements; the 16-byte vector kernels run when E, ldz and ldy are multiples of 16 / sizeof(T), z and y are
 * 16-byte aligned and E <= 1024 -- any other layout takes the scalar kernels, same results up to fp32 summation order. */
int mivit_layernorm_fwd(int dtype, const void *z, int64_t ldz, const float *gamma, const float *beta,
                        int M, int E, void *y, int64_t ldy, int rows_per_seq, int out_seq_stride, int out_row_off,
                        const float *pos, float *mean, float *rstd, void *stream);

/* dz = LayerNorm backward; dgamma/dbeta (+)= reductions over rows.  dy rows are read through the same row map
 * as the forward wrote them.  workspace: mivit_layernorm_bwd_workspace_bytes(M,E). */
size_t mivit_layernorm_bwd_workspace_bytes(int M, int E);
int mivit_layernorm_bwd(int dtype, const void *dy, int64_t lddy, const void *z, int64_t ldz,
                        const float *gamma, const float *mean, const float *rstd, int M, int E,
                        int rows_per_seq, int in_seq_stride, int in_row_off,
                        void *dz, int64_t lddz, float *dgamma, float *dbeta, int accumulate,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Multi-head self-attention core (models.py:42-54): per (b,h) softmax(q k^T / sqrt(Dh)) v, heads merged.
 * qkv: T [B*S, 3E] rows = [q | k | v] of one token (head h owns columns h*Dh..); ctx: T [B*S, E].
 * Whole sequences live in LDS (S <= mivit_attention_max_seq(dtype, Dh)). */
int mivit_attention_max_seq(int dtype, int Dh);
int mivit_attention_fwd(int dtype, const void *qkv, int B, int S, int H, int Dh, void *ctx, void *stream);
/* dqkv: T [B*S, 3E] from dctx T [B*S,E]; probabilities are recomputed from q,k (nothing saved). */
int mivit_attention_bwd(int dtype, const void *qkv, const void *dctx, int B, int S, int H, int Dh,
                        void *dqkv, void *stream);
/* The same when only the first q_rows query rows of every sequence carry a gradient: dctx holds q_rows rows of E per
 * sequence, dctx_seq_stride elements (a multiple of 8, >= q_rows * E) between sequences; the rows behind them are zero by
 * contract and never read.  All of dqkv [B*S, 3E] is written (dq of the other query rows as zeros) and equals what
 * mivit_attention_bwd makes of the zero-padded dctx.  16-bit dtypes, S <= 128, head dim 16 / 32 / 64 (the short-sequence
 * kernel); an error elsewhere and under MIVIT_ATTN_BWD=1. */
int mivit_attention_bwd_rows(int dtype, const void *qkv, const void *dctx, int64_t dctx_seq_stride, int q_rows, int B, int S,
                             int H, int Dh, void *dqkv, void *stream);
/* The same reading less: of q only the first q_rows rows of a sequence are read (every other query row has dS = 0 whatever its
 * scores are: zeros stand in for it).  dqkv is bitwise that of mivit_attention_bwd_rows. */
int mivit_attention_bwd_rows_lean(int dtype, const void *qkv, const void *dctx, int64_t dctx_seq_stride, int q_rows, int B, int S,
                                  int H, int Dh, void *dqkv, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Model level: GeneralTransformer.forward / its autograd (models.py:278-361, :111-141, :81-108).
 * Parameters live in ONE fp32 arena whose layout the plan defines (so q/k/v weights are contiguous and the
 * gradient arena can be all-reduced per stage without copies).  Names are the reference state-dict keys.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mivit_config {
    int abi_version;       /* = MIVIT_ABI_VERSION */
    int dtype;             /* MIVIT_F32 | MIVIT_BF16 */
    int embedding;         /* MIVIT_EMBED_LINEAR | _CNN (same arithmetic, weight viewed [E,P*P]) | _EXTERNAL
                              (caller supplies pre-LayerNorm tokens [B,T,E], e.g. DeepResNetEmbedding) */
    int patch_size;        /* P: frame side; a token is a whole frame */
    int embed_dim;         /* E */
    int num_heads;         /* H */
    int hidden_dim;        /* F */
    int num_layers;        /* L */
    int activation;        /* MIVIT_ACT_* for FeedForward */
    int use_pos_encoding;  /* learned [1,128,E] table */
    int use_regression_token;
    int fusion;            /* MIVIT_FUSION_* */
    int global_feature_dim;
    int head_hidden;       /* MLPHead hidden (128) */
    int output_dim;        /* MLPHead outputs (1) */
} mivit_config;

typedef struct mivit_plan mivit_plan;

mivit_plan *mivit_plan_create(const mivit_config *cfg);   /* NULL on error */
void mivit_plan_destroy(mivit_plan *plan);

/* Parameter arena layout (floats). */
int mivit_plan_num_params(const mivit_plan *plan);
const char *mivit_plan_param_name(const mivit_plan *plan, int i);   /* reference state-dict key */
int64_t mivit_plan_param_offset(const mivit_plan *plan, int i);     /* float offset into the arena */
int64_t mivit_plan_param_numel(const mivit_plan *plan, int i);
int64_t mivit_plan_arena_numel(const mivit_plan *plan);
/* Backward stages, in execution order: 0 = head(+final norm, feature projector), 1..L = encoder layers
 * L-1..0, L+1 = token assembly + embedding.  Stage s owns arena floats [begin,end): its gradients are final
 * once mivit_backward(.., s, s+1, ..) has been enqueued -- this is what the data-parallel host overlaps
 * its per-stage all-reduce with. */
int mivit_plan_num_stages(const mivit_plan *plan);
int mivit_plan_stage_range(const mivit_plan *plan, int stage, int64_t *begin, int64_t *end);

size_t mivit_plan_workspace_bytes(const mivit_plan *plan, int B, int T, int need_backward);

/* x: fp32 [B,T,P,P] frames (or fp32 [B,T,E] pre-norm tokens for _EXTERNAL); features: fp32 [B,Fg] or NULL;
 * out: fp32 [B,output_dim].  The workspace keeps what backward needs; it must stay untouched until then. */
int mivit_forward(const mivit_plan *plan, const float *params, const float *x, const float *features,
                  int B, int T, void *workspace, size_t workspace_bytes, int need_backward,
                  float *out, void *stream);

/* Runs backward stages [stage_begin, stage_end).  dout: fp32 [B,output_dim].  grads: fp32 arena, same
 * layout as params; every parameter element of a stage's range is OVERWRITTEN (no accumulation; the rows of
 * transformer.pos_embedding beyond the sequence with 0), the alignment padding between tensors is never
 * written.  dfeatures (fp32 [B,Fg]) and dx_tokens (fp32 [B,T,E], _EXTERNAL only) may be NULL when not needed. */
int mivit_backward(const mivit_plan *plan, const float *params, const float *x, const float *features,
                   int B, int T, void *workspace, size_t workspace_bytes, const float *dout,
                   float *grads, float *dfeatures, float *dx_tokens,
                   int stage_begin, int stage_end, void *stream);

/* hipGraph replay statistics.  mivit_forward / mivit_backward / mivit_deepresnet_train_* on small (launch-bound) problems
 * capture their kernel sequence into a hipGraph the second time they see the same arguments and replay it afterwards
 * (MIVIT_GRAPHS=0 disables; off while mivit_profile_enable is active).  A replay reads the current contents of every buffer:
 * only addresses, sizes and the launch sequence are frozen.  Changing any mivit_*_set_* switch starts the affected keys over
 * (the next call runs directly, the one after is captured under the new value). */
void mivit_graph_stats(uint64_t *replays, uint64_t *captures, int *failures);

/* Readout-row pruning of the last encoder layer (fused 16-bit layers with the regression-token readout, more than one token):
 * the head reads B of its B * S output rows.
 *   1 (default): the last feed-forward block's forward runs on those B rows and the attention core's backward on the one query
 *      row per sequence that carries a gradient; the last attention block computes its query side for the first row tile only,
 *      and its LayerNorm-1 / out-projection and attention-core backward do not read the rows in which d(x1) is an exact zero
 *      or whose q only ever multiplies one.  Every result is what it was: no sum changes its terms or their order.
 *   3: mode 1 without the second sentence (the launches mode 1 made before the readout query; A/B runs and tests).
 *   2 (MIVIT_READOUT_ROWS=2): the feed-forward block's and LayerNorm-1 / out-projection's backward run on B rows too.  Same out
 *      and loss; the last layer's fc1 / fc2 / norm2 / out_proj / norm1 gradients sum the same fp32 terms in another order, which
 *      a training run amplifies like any other rounding difference.
 *   0 (MIVIT_NO_READOUT_ROWS): every row.
 * Returns the previous value.  A forward and the backward that follows it must run under the same value. */
int mivit_set_readout_rows(int mode);

/* ------------------------------------------------------------------------------------------------
 * In-library kernel timing (used by bench.py for the roofline line): when a tag's bit is set in `tag_mask`, the
 * MAIN kernel of every launch in that category is bracketed by a hipEvent pair on the launch stream.
 * mivit_profile_collect waits for the recorded events, returns their summed duration and count, and resets
 * the tag.  Tags refer to the model-level engine's launches (operator-level calls are tagged MIVIT_PROF_OP).
 * ---------------------------------------------------------------------------------------------- */
enum {
    MIVIT_PROF_EMBED_FWD = 0,   /* patch-embedding GEMM  [B*T,P*P] x [E,P*P]^T            (HBM-bound)  */
    MIVIT_PROF_EMBED_WGRAD = 1, /* its weight gradient   d_emb^T x, re-reads the frames  (HBM-bound)  */
    MIVIT_PROF_LINEAR_FWD = 2,  /* qkv / out-proj / fc1 / fc2 / head forward GEMMs                     */
    MIVIT_PROF_LINEAR_DGRAD = 3,
    MIVIT_PROF_LINEAR_WGRAD = 4,
    MIVIT_PROF_ATTN_FWD = 5,
    MIVIT_PROF_ATTN_BWD = 6,
    MIVIT_PROF_LN_FWD = 7,
    MIVIT_PROF_LN_BWD = 8,
    MIVIT_PROF_OP = 9,
    /* the launches of the fused encoder-layer path (bf16, E 128 / F 256 / 4 heads), one tag per kernel: */
    MIVIT_PROF_ATTN_BLOCK_FWD = 10, /* LayerNorm affine + q|k|v + attention + out-proj + residual + LayerNorm-1 (fused_fwd.hip) */
    MIVIT_PROF_MLP_BLOCK_FWD = 11,  /* fc1 + activation + fc2 + residual + LayerNorm-2                                    */
    MIVIT_PROF_MLP_BLOCK_BWD = 12,  /* their backward incl. all six parameter gradients (fused_bwd.hip)                   */
    MIVIT_PROF_ATTN_OUT_BWD = 13,   /* LayerNorm-1 backward + out-projection data / weight gradient                       */
    MIVIT_PROF_ATTN_CORE_BWD = 14,  /* attention core backward (attention_fast.hip)                                       */
    MIVIT_PROF_QKV_WGRAD = 15,      /* q|k|v weight gradient (wgrad_dma.hip) + affine fix-up                              */
    MIVIT_PROF_QKV_DGRAD = 16,      /* q|k|v data gradient + residual gradient (rowstream.hip)                            */
    MIVIT_PROF_QKV_BWD = 17,        /* both of them in one pass over dqkv (fused_bwd.hip::qkv_bwd_kernel) + affine fix-up  */
    MIVIT_PROF_NUM_TAGS = 18
};
int mivit_profile_enable(uint64_t tag_mask);   /* 0 disables */
int mivit_profile_collect(int tag, double *total_ms, int *count);
const char *mivit_profile_tag_name(int tag);

#ifdef __cplusplus
}
#endif
#endif /* MIVIT_HIP_H */
