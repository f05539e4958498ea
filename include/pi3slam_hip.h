/* pi3slam_hip.h — C ABI of libpi3slam_hip.so: the gfx950 (MI355X) kernels of the Pi3-SLAM hot path.
 *
 * The reference (urbste/Pi3_SLAM) is pure Python on PyTorch; its only native FFI is the optional pybind11 module
 * `curope` with one function rope_2d(tokens, positions, base, fwd) (pi3/models/curope/curope.cpp:49-68,
 * kernels.cu:17-108), which its own entry points never load.  Everything else on the path is a torch operator call.
 * This header is therefore the boundary a maintainer binds with ctypes: each entry point names
 * the reference call site (file:line) whose arithmetic it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless the name ends in `_host`;
 *   - no allocation, no host synchronisation, no implicit stream: the caller passes a hipStream_t as `void* stream`
 *     (0 = default stream); calls are asynchronous and re-entrant per stream;
 *   - return 0 on success, negative on error (PI3_ERR_*); pi3_last_error() returns the thread-local message;
 *   - row-major tensors; `ld*` / strides are in ELEMENTS; bf16 = 16-bit brain float, f16 = IEEE half;
 *   - dtype codes: 0 = bf16, 1 = f32, 2 = f16 (IEEE half: the MoGe path, which the reference runs under fp16
 *     autocast; entries that take it say so).
 */
#ifndef PI3SLAM_HIP_H
#define PI3SLAM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PI3_OK 0
#define PI3_ERR_ARG (-1)
#define PI3_ERR_LAUNCH (-2)
#define PI3_ERR_WORKSPACE (-3)

const char* pi3_last_error(void);
int pi3_abi_version(void);   /* 7 */
const char* pi3_build_flavor(void);   /* "product" | "dev" (make dev: development variants and timing ablations compiled in) */

/* Run-time A/B knob (speed only: every value selects a correct variant).  The product library knows four names:
 * attn_asm (0 | 2), attn_nomax (0 | 1 | 2), gelu_form (0 | 1), ba_schur_rows (0 | 1) - see csrc/api.hip; a development
 * build adds the measured-slower forms (gemm_4w, gemm_ilv, gemm_stagger_ns, gemm_rpref, attn_frame_nw).  Any other name is
 * refused with PI3_ERR_ARG.  The environment variable PI3_<NAME> is a knob's initial value.  Used by tools/ and the
 * tests to interleave variants in one process. */
int pi3_set_knob(const char* name, long value);
/* 1 and *value if the knob has a value, 0 if unset (launch paths use their defaults), PI3_ERR_ARG for an unknown name */
int pi3_get_knob(const char* name, long* value);
int pi3_unset_knob(const char* name);
int pi3_device_count(void);

/* ---- transformer blocks -------------------------------------------------------------------------------------- */

/* torch.nn.Linear with fused epilogue (pi3/models/layers/block.py:310-335, pi3/models/dinov2/layers/mlp.py:34-40,
 * pi3/models/layers/attention.py:325,345, transformer_head.py:49,55,74, camera_head.py:26-31, patch_embed.py:75):
 *   out[orow(m)][n] = resid[orow(m)][n] + gamma[n] * act((A[m] . W[n] + bias[n]) * (n < qcols ? qscale : 1))
 *                     + addtab[m % rpg][n]
 *   orow(m) = rpg ? (m / rpg) * gstride + goff + m % rpg : m.   bias/gamma/resid/addtab may be NULL.
 * A [M][K] and W [N][K] share in_dtype (0: bf16 MFMA, 1: exact-fp32 MFMA, 2: f16 MFMA - then out_dtype is 2 or 1);
 * N % 128 == 0, or with 16-bit operands any N % 32 == 0 (32 / 64-column tiles: the narrow maps of the MoGe pyramid); K % 64 (bf16) / 32 (f32).
 * act: 0 none, 1 GELU(erf), 2 ReLU.
 * qcols: a multiple of 4 with 0 <= qcols <= N (the epilogue scales whole groups of 4 columns); anything else is
 * refused with PI3_ERR_ARG before any launch. */
int pi3_gemm(const void* A, long lda, const void* W, long ldw, int M, int N, int K, int in_dtype, const float* bias,
             const float* gamma, const float* resid, long ldr, void* out, long ldo, int out_dtype, int act, int rpg,
             int gstride, int goff, const float* addtab, long ldadd, float qscale, int qcols, void* stream);

/* The packed qkv projection of a transformer block with everything FlashAttentionRope.forward does to q and k before the
 * attention call fused into its epilogue (pi3/models/layers/attention.py:323-334; replaces the reference's
 * nn.Linear + q_norm / k_norm LayerNorm(64) + RoPE2D (= the optional curope.rope_2d, pi3/models/curope/curope.cpp:49-68)
 * + the softmax scale):
 *   qkv[M][3*H*64] bf16 = A[M][K] . W[3*H*64][K]^T + bias;  per head of q and k: LayerNorm over the 64 dims (eps; only
 *   when qw/qb/kw/kb are given), RoPE-2D with positions pos[row % T] = (y, x) and the table cs[npos][16][2] = (cos, sin)
 *   (only when pos/cs are given), q *= qscale.
 * k2max (optional, attn_B*H floats, caller-owned): receives max_s |k[b, s, h, :]|^2 for the attention call that follows
 * (rows = attn_B batches of attn_S tokens) - pass it to pi3_attention with k2max_ready = 1. */
int pi3_gemm_qkv(const void* A, long lda, const void* W, long ldw, int M, int K, int H, const float* bias, void* qkv,
                 long ldo, int T, const int* pos, const float* cs, const float* qw, const float* qb, const float* kw,
                 const float* kb, float eps, float qscale, float* k2max, int attn_B, int attn_S, void* stream);

/* F.scaled_dot_product_attention, non-causal, head_dim 64 (pi3/models/layers/attention.py:102-107, 336-341).
 * q/k/v: bf16, element (b, s, h, d) at ptr[b*batch_stride + s*tok_stride + h*64 + d]; q PRE-SCALED by
 * 64^-0.5 * log2(e).  o: bf16 [B][S][H*64] with the given strides.
 * o must not overlap q/k/v.
 * k2max_ws: caller-provided workspace of B*H floats (this library allocates nothing) for max_s |k[b,s,h,:]|^2, or
 * NULL.  With it the 64-row kernel keeps its bounded-score loop (no running max) without further ado for every wave
 * whose scores are provably inside the fp32/bf16 exponent range (|q| max|k| <= 90 in the exp2 domain).  Other waves -
 * all of them when NULL - run the same loop optimistically (knob attn_nomax = 2, the default): their workgroup keeps
 * the result iff every row sum lies in [2^-60, 2^120] and the outputs are finite, else a second launch inside this call
 * recomputes that workgroup on the online-max loop (attn64.hip, a64_reject).  Knob 1: waves outside the bound go to
 * the online-max loop directly (rounds 3-4); 0: online-max loop everywhere.  Every form is the exact softmax.
 * k2max_ready = 0: the call zeroes the workspace and fills it with a pre-pass over k; 1: the workspace already
 * holds the maxima (written by pi3_gemm's fused q/k epilogue, see pi3_gemm_qkv).
 * dtype: 0 = q/k/v/o bf16 (pi3), 2 = IEEE half (MoGe: the reference runs it under fp16 autocast, moge/model/v2.py:228):
 * the same kernel on v_mfma_f32_32x32x16_f16, online-max loop only (half has 5 exponent bits), k2max_ws unused. */
int pi3_attention(const void* q, const void* k, const void* v, long tok_stride, long batch_stride, void* o,
                  long o_tok_stride, long o_batch_stride, int B, int S, int H, int head_dim, int dtype, float* k2max_ws,
                  int k2max_ready, void* stream);

/* Diagnostic of pi3_attention's long-sequence kernel: which softmax loop its waves took.  counters: caller-owned DEVICE
 * memory of 128 uint32, zeroed by the caller, laid out [kind][path][32 slots] (sum the slots): kind 0 = eight-wave
 * workgroups (global attention), 1 = four-/two-wave workgroups (frame-wise attention); path 0 = the wave's result comes
 * from the bounded-score loop, 1 = from the online-max loop (under knob attn_nomax = 2 these are the waves of workgroups
 * that rejected the optimistic pass and ran again).  bf16 launches only: the IEEE-half form (MoGe) has one loop and is
 * not counted (until round 5's last build its waves appeared under kind 1 / path 1: the "0.4 % online-max" of the
 * frame-wise line in earlier bench records was MoGe's encoder, not pi3's).  One no-return atomic per wave while registered; NULL (the default) switches it off.
 * Process-wide; change it only while no attention launch is in flight.  bench.py reports the fractions with it. */
int pi3_attention_path_counters(unsigned int* counters);

/* nn.LayerNorm(D, eps) over rows of x (block.py:282,296; vision_transformer.py:271).  If nspecial > 0 (f32 out only),
 * rows with (row % T) < nspecial are replaced by special[row % T][:]: Pi3.decode's register-token concat
 * (pi3/models/pi3.py:140-144). */
int pi3_layernorm(const float* x, long ldx, int rows, int D, const float* w, const float* b, float eps, void* out,
                  long ldo, int out_dtype, int T, int nspecial, const float* special, void* stream);

/* In place on packed qkv bf16 [rows][3][H][64]: optional LayerNorm(64) of q and k (attention.py:330), RoPE-2D
 * (pos_embed.py:142-159 == curope.cpp:11-47; pos int32 [T][2] (y, x) indexed by row % T; cs f32 [npos][16][2] =
 * (cos, sin) of pos * base^(-j/16)), then q *= qscale.  The two-pass form of pi3_gemm_qkv's epilogue (a different
 * contract from the reference's `curope.rope_2d`: that one is pi3_rope_2d below). */
int pi3_qknorm_rope(void* qkv, long rows, int H, int T, const int* pos, const float* cs, const float* qw,
                    const float* qb, const float* kw, const float* kb, float eps, float qscale, int do_rope,
                    void* stream);

/* The reference's one native FFI entry under its own contract: `curope.rope_2d(tokens, positions, base, fwd)`
 * (pi3/models/curope/curope.cpp:49-68, kernels.cu:17-108), what `cuRoPE2D.forward` (curope2d.py:33-40) calls.
 * In place on tokens (B, N, H, D): element (b, n, h, d) at tokens[b*stride_b + n*stride_n + h*stride_h + d] (the last
 * dim contiguous; 0 for a stride = the contiguous default D, H*stride_h, N*stride_n.  kernels.cu:91 also demands
 * stride_h == D, which excludes the transposed view of a contiguous (B, heads, N, D) tensor that `cuRoPE2D.forward`
 * produces behind pi3's q_norm: accepted here);
 * positions int64 (B, N, 2) = (y, x), contiguous; D % 4 == 0.  With Q = D/4 a token vector is [u_Y | v_Y | u_X | v_X]:
 *   freq = pos * fwd / base^(d/Q);   u' = u cos(freq) - v sin(freq);   v' = v cos(freq) + u sin(freq)     (fp32)
 * fwd = F0 (1.0) rotates forward, -F0 is the reference's backward pass = the inverse rotation.
 * dtype of tokens: 0 = bf16, 1 = f32, 2 = f16 (kernels.cu:103 dispatches over floating types + Half + BFloat16).
 * The hot path does not call it (the rotation rides in pi3_gemm_qkv's epilogue); it exists so that a `cuRoPE2D`
 * caller binds to this library unchanged. */
int pi3_rope_2d(void* tokens, const long* positions, int B, int N, int H, int D, long stride_b, long stride_n,
                long stride_h, float base, float fwd, int dtype, void* stream);

/* f32 -> bf16/f32 strided row copy (concat of the last two decoder outputs, pi3.py:168-171). */
int pi3_cast_rows(const float* in, long ldi, void* out, long ldo, long rows, int cols, int out_dtype, void* stream);
/* same, reading only the first in_cols columns of a row and writing zeros in [in_cols, cols): the K padding of the GEMM
 * that follows a narrow MoGe map (moge/model/modules.py:242-254 feeds 32-channel maps to 1x1 convolutions). */
int pi3_cast_rows_pad(const float* in, long ldi, int in_cols, void* out, long ldo, long rows, int cols, int out_dtype,
                      void* stream);

/* frames f32 [F][3][H][W] -> ImageNet-normalised (pi3.py:174) bf16 patch rows [F*P][KP], column c*196 + ky*14 + kx,
 * zero padded to KP: the im2col of PatchEmbed's Conv2d (patch_embed.py:65,75).  mean3/std3 are HOST arrays.
 * out_dtype: 0 bf16, 2 f16. */
int pi3_patch_gather(const float* img, int F, int H, int W, void* out, int KP, int out_dtype, const float* mean3_host,
                     const float* std3_host, void* stream);

/* dst[oy][ox][:] = sum_ij wy[oy][i] wx[ox][j] src[i][j][:]: bicubic-antialias resample of pos_embed
 * (vision_transformer.py:205-210) with host-built tap matrices. */
int pi3_resample_grid(const float* src, int Mi, int Mj, int D, const float* wy, const float* wx, int oh, int ow,
                      float* dst, void* stream);

/* x[(f*T + t0 + t)][:] = vals[t][:] for t < nt (cls + registers, vision_transformer.py:221-232). */
int pi3_fill_tokens(float* x, int F, int T, int D, int t0, int nt, const float* vals, void* stream);

/* Recipe weights (no checkpoint exists offline): out[i] = offset + scale * u(seed, i), bit-identical to
 * pi3_slam_amd/recipe.py. */
int pi3_recipe_fill(void* out, long n, unsigned long long seed, float offset, float scale, int out_dtype,
                    void* stream);

/* ---- output heads --------------------------------------------------------------------------------------------- */

/* LinearPts3d's pixel_shuffle + remap + unprojection (transformer_head.py:76-80, pi3.py:195-209).  Feature row of
 * frame f, patch p is f*T + tok_off + p.  Outputs f32 [F][H][W][3], [F][H][W][3], [F][H][W][1]. */
int pi3_unpatchify_points(const float* pfeat, long ldp, const float* cfeat, long ldc, const float* poses, int F,
                          int H, int W, int T, int tok_off, float* local_points, float* points, float* conf,
                          void* stream);

/* CameraHead after the ResConv blocks (camera_head.py:55-93): token mean, 2x Linear+ReLU, fc_t, fc_rot, SO(3)
 * projection -> poses f32 [F][4][4] cam->world. */
int pi3_camera_tail(const float* feat, long ld, long frame_stride, int F, int P, int D, const float* w1,
                    const float* b1, const float* w2, const float* b2, const float* wt, const float* bt,
                    const float* wr, const float* br, float* poses, void* stream);

/* ---- per-chunk post-processing ------------------------------------------------------------------------------- */

/* masks = sigmoid(conf) > conf_thr & ~depth_edge(z, rtol) (slam/offline_chunk_creator.py:114-119,
 * pi3/utils/geometry.py:347-375).  masks: uint8 [F][H][W]. */
int pi3_compute_masks(const float* conf, const float* local_points, int F, int H, int W, float conf_thr, float rtol,
                      unsigned char* masks, void* stream);

/* out2[0] = lower median of (num[i] / den[i*den_stride]) over mask[i] != 0, out2[1] = count
 * (_get_scale_factor_for_pi3, offline_chunk_creator.py:121-127). */
int pi3_masked_ratio_median(const float* num, const float* den, long den_stride, const unsigned char* mask, long n,
                            float* out2, void* stream);

/* local_points *= s; points *= s; poses[:, :3, 3] *= s with s = *scale_dev (offline_chunk_creator.py:189-191). */
int pi3_apply_scale(const float* scale_dev, float* local_points, float* points, long n3, float* poses, int F,
                    void* stream);

/* grid_sample of the dense maps at keypoints + fp16 pack (offline_chunk_creator.py:129-159, 231-241;
 * utils/keypoint_extraction.py:203-229).  keypoints f32 [F][K][2] (x, y) px; images f32 [F][3][H][W] or NULL.
 * Outputs: f16 [F][K][3], f16 [F][K][3], f16 [F][K][1], uint8 [F][K][1], f16 [F][K][3] (0..255), f16 [F][K][2]. */
int pi3_gather_keypoints(const float* points, const float* local_points, const float* conf,
                         const unsigned char* masks, const float* images, const float* keypoints, int F, int H,
                         int W, int K, void* o_points, void* o_local, void* o_conf, unsigned char* o_mask,
                         void* o_colors, void* o_kps, void* stream);

/* Per-frame focal / z-shift + intrinsics (utils/camera_estimation.py:12-70, utils/geometry_torch.py:114-169,
 * utils/geometry_numpy.py:79-96: scipy least_squares(method='lm') == MINPACK lmdif, n = 1).  uvx [W], uvy [H]: fp32
 * normalized_view_plane_uv tables.  Pixel validity: mask8 (uint8, if not NULL) else sigmoid(conf) > conf_thr.  Outputs f32: focal [F], shift [F], (fx, fy, cx, cy) [F][4], K [F][3][3]. */
int pi3_focal_shift(const float* local_points, const float* conf, const unsigned char* mask8, const float* uvx,
                    const float* uvy, int F, int H, int W, float conf_thr, float* focal, float* shift,
                    float* fxfycxcy, float* K33, void* stream);

/* ---- MoGe-2 metric-scale forward (moge/model/v2.py:128-290, moge/model/modules.py:18-254) ------------------------ */

/* nn.Conv2d(C, N, 3, padding=1, padding_mode='replicate') as an implicit GEMM on a bf16 NHWC image [B][H][W][ldc];
 * out rows = pixels; epilogue bias / resid / act; N % 32 == 0.
 *   C % 64 == 0: wgt bf16 [N][9*C], k = (ky*3+kx)*C + ci;
 *   C == 32:     wgt bf16 [N][10*32], k = tap*32 + ci with a tenth, all-zero tap (two taps per 64-wide K-step).
 * in_dtype: 0 = image and weights bf16, 2 = IEEE half; out_dtype: 1 = f32, or the image's 16-bit type. */
int pi3_conv3x3(const void* img, long ldc, int B, int H, int W, int C, const void* wgt, int N, const float* bias,
                const float* resid, long ldr, void* out, long ldo, int in_dtype, int out_dtype, int act, void* stream);

/* nn.GroupNorm(G, C) statistics of x f32 [B][HW][ldx] -> stats f64 [B][G][2] (sum, sum of squares).  Deterministic
 * two-pass reduction (no floating-point atomics) through the caller's workspace ws of at least
 * pi3_groupnorm_ws_doubles(B, HW, C) doubles. */
long pi3_groupnorm_ws_doubles(int B, int HW, int C);
int pi3_groupnorm_stats(const float* x, long ldx, int B, int HW, int C, int G, double* stats, double* ws,
                        long ws_doubles, void* stream);

/* Norm + activation in front of a ResidualConvBlock convolution (moge/model/modules.py:47-58) -> bf16 NHWC staging
 * image [B][HW][ldo], channels [C, Cpad) zeroed (Cpad % 4 == 0, ldo % 4 == 0).  G groups (GroupNorm(C/32), 'layer_norm' = 1 group, InstanceNorm2d =
 * C groups with gamma = beta = NULL); G = 0: no normalisation ('none').  act: 0 none, 2 ReLU, 3 LeakyReLU(0.2),
 * 4 SiLU, 5 ELU.  out_dtype: 0 bf16, 2 f16. */
int pi3_groupnorm_apply(const float* x, long ldx, int B, int HW, int C, int Cpad, int G, const double* stats,
                        const float* gamma, const float* beta, float eps, int act, void* out, long ldo, int out_dtype,
                        void* stream);

/* x[r][0..C) += y[r][0..C) on fp32 maps: ConvStack with an identity input block (modules.py:245-249). */
int pi3_add_rows(float* x, long ldx, const float* y, long ldy, long rows, int C, void* stream);

/* ConvTranspose2d(k=2, s=2) scatter: g f32 [B*H*W][(dy*2+dx)*Cs + co] -> bf16 NHWC [B][2H][2W][ldo], channels
 * [Cout, Cpad) zeroed (Cpad % 4 == 0, ldo % 4 == 0).  out_dtype: 0 bf16, 2 f16. */
int pi3_convt_scatter(const float* g, long ldg, int B, int H, int W, int Cout, int Cs, int Cpad, void* out, long ldo,
                      int out_dtype, void* stream);

/* x[b][y][x][c] (+)= w[c][wofs] * uvx[x] + w[c][wofs+1] * uvy[y] + bias[c]: 1x1 conv of the UV planes (v2.py:141-147). */
int pi3_uv_affine(float* x, long ldx, int B, int H, int W, int C, const float* w, long ldw, int wofs,
                  const float* bias, const float* uvx, const float* uvy, int accumulate, void* stream);

/* Separable resize with host-built tap tables (ys/xs int32 [o][2] = start,count; yw/xw f32 [o][8]); generic strides. */
int pi3_resize_taps(const float* src, long sc, long sy, long sx, int C, const int* ys, const float* yw, const int* xs,
                    const float* xw, int oh, int ow, float* dst, long dc, long dy, long dx, void* stream);

/* y = act(W x + b) for a single vector (scale_head MLP, modules.py:184-192). */
int pi3_dense_vec(const float* x, const float* Wt, const float* b, int K, int N, int act, float* y, void* stream);

/* In-place point remap (0 linear, 1 exp, 2 sinh, 3 sinh_exp) + binary mask = sigmoid(logit) > 0.5 (v2.py:160-170, 241). */
int pi3_moge_remap(float* pts, const float* mask_logit, long n, int remap, unsigned char* mask, void* stream);

/* depth = z + *shift; mask &= depth > 0; depth *= exp(*log_scale); depth = mask ? depth : inf (v2.py:255-274). */
int pi3_moge_depth(const float* pts, const float* shift, const float* log_scale, unsigned char* mask, long n,
                   float* depth, void* stream);

/* ---- overlap Sim(3) alignment (utils/reconstruction_alignment.py:74-105) --------------------------------------- */

/* idx[v][j] = index of the ref keypoint with bit-identical f16 (x, y) in overlap view v, or -1 (:74). */
int pi3_sim3_match_keypoints(const void* kp_ref, const void* kp_qry, int ov, int K, int* idx, void* stream);

/* Near-half filter (:78-86, use_filter != 0) + closed-form Umeyama similarity qry -> ref (:89-105).
 * pts_*: [ov][K][3], f16 as chunk files store them, or f32 when bit 1 of use_filter is set (bundle-adjusted chunks);
 * w_*: optional uint8 validity [ov][K]; last_ref_pose: f32 [16] cam->world of the last ref view.
 * out33 (f64): [0] s, [1..9] R, [10..12] t, [13..28] 4x4, [29] pairs used, [30] common pairs, [31] median, [32] rms. */
int pi3_sim3_umeyama(const void* pts_ref, const void* pts_qry, const int* idx, const unsigned char* w_ref,
                     const unsigned char* w_qry, int ov, int K, const float* last_ref_pose, int use_filter,
                     double* out33, void* stream);

/* The same solve with real-valued weights w_*: f32 [ov][K] (either may be null = 1): the "weighted Umeyama" of the
 * north star (w = mask * sigmoid(conf)).  Pair weight = w_ref[ref track] * w_qry[qry keypoint];
 * pairs whose weight is not in (0, inf) do not take part; W = sum w, weighted means / covariance / variance / rms; the
 * near-half filter is the reference's unweighted median over the pairs that take part.  The reference itself passes
 * unweighted points (utils/reconstruction_alignment.py:97), so the host code keeps this off by default. */
int pi3_sim3_umeyama_weighted(const void* pts_ref, const void* pts_qry, const int* idx, const float* w_ref,
                              const float* w_qry, int ov, int K, const float* last_ref_pose, int use_filter,
                              double* out33, void* stream);

/* TransformReconstruction4 (:105): points f32 [n][3] and cam->world poses f32 [F][16] in place by the f64 4x4. */
int pi3_sim3_apply(const double* M4_dev, float* pts, long n, float* poses, int F, void* stream);

/* G[c] = G[c-1] . T[c], G[0] = T[0]: prefix composition of per-chunk relative similarities ([n][16] f64). */
int pi3_sim3_compose_prefix(const double* T, double* G, int n, void* stream);

/* ---- next-tier: observation projection of ChunkPTRecon (utils/chunk_reconstruction.py:162-185,
 * 445-509).  points f16 [N][K][3], poses f32 [N][16], intrinsics f32 [N][9] -> uv f32 [N][N][K][2] ([source][target]),
 * valid uint8 [N][N][K] (in-bounds observations of the pairs target < source or source < target <= source + max_after). */
int pi3_project_observations(const void* points, const float* poses, const float* intrinsics, int N, int K, int W,
                             int H, int max_after, float* uv, unsigned char* valid, void* stream);

/* ---- next-tier: frame ingest = Resize + ToTensor of ChunkImageDataset._load_image_chunk
 * (datasets/image_datasets.py:186-208), bit-exact with Pillow's 8-bit bilinear resample.  src u8 [N][H0][W0][3];
 * x/y bounds int32 [out][2] = (first tap, taps), coefs int32 [out][ksize] (22-bit fixed point, built on the host);
 * tmp u8 [N][H0][W1][3] workspace; dst f32 [N][3][H1][W1] in [0, 1]. */
int pi3_ingest_frames(const unsigned char* src, int N, int H0, int W0, int H1, int W1, const int* xbounds,
                      const int* xcoefs, int xksize, const int* ybounds, const int* ycoefs, int yksize,
                      unsigned char* tmp, float* dst, void* stream);

/* ---- next-tier: undistortion of the input frames (pi3/utils/undistortion.py:95-138, :157-177).
 * pi3_undistort_maps: params is a HOST pointer to 16 doubles (undistorted camera f, aspect, cx, cy, skew; distorted
 * camera f, aspect, cx, cy, skew; radial k1..k4; tangential t1, t2); model 0 PINHOLE, 1 PINHOLE_RADIAL_TANGENTIAL,
 * 2 FISHEYE, 3 DIVISION_UNDISTORTION; map_x / map_y f32 [H][W] device (source pixel of every target pixel).
 * pi3_remap_bilinear_u8: cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) of src u8 [N][H0][W0][3] + ToTensor ->
 * dst f32 [N][3][H][W]. */
int pi3_undistort_maps(const double* params, int model, int H, int W, float* map_x, float* map_y, void* stream);
int pi3_remap_bilinear_u8(const unsigned char* src, int N, int H0, int W0, const float* map_x, const float* map_y,
                          int H, int W, float* dst, void* stream);

/* ---- bundle adjustment of a chunk ---------------------------------------------------------- */

/* Replaces pt.sfm.BundleAdjustReconstruction as the reference configures it (utils/chunk_reconstruction.py:188-209:
 * 10 iterations, Huber 2.0, DENSE_SCHUR; utils/reconstruction_alignment.py:137-159: 50 iterations, Huber 3.0, with the
 * orientation / position priors of :110-132).  pytheia / Ceres are not available offline: restated algorithm, parity
 * unpinned (see csrc/ba.hip).  Dense problem layout: track (s, k), observed by camera t iff valid[s][t][k];
 * uv [N][N][K][2] f32 pixels (the diagonal t == s = the keypoint itself), uvT / validT = the same with the last two
 * index axes swapped ([N][K][N]).  points f64 [N*K][3] and poses f64 [N][12] = [R world->camera (9) | centre (3)] are
 * refined IN PLACE; intr f64 [N][4] = fx, fy, cx, cy (fixed).  prior_flag (or NULL) marks cameras with a pose prior
 * (prior_R [N][9], prior_C [N][3]); sqrt_info_* = 1 / sqrt(covariance).  summary_dev: 11 doubles (cost, candidate
 * cost, radius, decrease factor, model decrease, iterations, accepted steps, done, initial cost, cholesky failure,
 * last step accepted).  N <= 128.  workspace: pi3_ba_workspace_doubles(N, K) doubles. */
long pi3_ba_workspace_doubles(int N, int K);
int pi3_bundle_adjust(double* points, double* poses, const double* intr, const float* uv, const unsigned char* valid,
                      const float* uvT, const unsigned char* validT, int N, int K, double huber_width, int max_iters,
                      const double* prior_R, const double* prior_C, const unsigned char* prior_flag,
                      double sqrt_info_rot, double sqrt_info_pos, double* summary_dev, double* workspace,
                      long workspace_doubles, void* stream);

/* The same adjustment with the point parametrization the reference's two calls configure
 * (ba_options.use_homogeneous_point_parametrization = True: utils/reconstruction_alignment.py:147-152,
 * utils/chunk_reconstruction.py:199-204): every track is the 4-vector [X, 1] / |[X, 1]| stepped in the tangent space of
 * its unit sphere (ceres::HomogeneousVectorParameterization: Householder basis, Plus).  Same objective and optimum as
 * pi3_bundle_adjust (Euclidean steps); the LM damping acts in different coordinates, so the iterates differ
 * (tests/test_ba_oracle.py).  Same arguments, same workspace size. */
int pi3_bundle_adjust_homogeneous(double* points, double* poses, const double* intr, const float* uv,
                                  const unsigned char* valid, const float* uvT, const unsigned char* validT, int N, int K,
                                  double huber_width, int max_iters, const double* prior_R, const double* prior_C,
                                  const unsigned char* prior_flag, double sqrt_info_rot, double sqrt_info_pos,
                                  double* summary_dev, double* workspace, long workspace_doubles, void* stream);

/* The reference's --use-inverse-depth (reconstruction.InitializeInverseDepth() + ba_options.use_inverse_depth_parametrization
 * = True: utils/chunk_reconstruction.py:187-204, utils/reconstruction_alignment.py:147-152): every track (s, k) is ONE
 * parameter, the inverse depth along the bearing of its keypoint in its reference view s (its own frame),
 * X = C_s + R_s^T (b / rho); observations by other cameras depend on (pose_t, pose_s, rho), the reference view's own
 * observation carries no residual.  `points` are snapped onto those rays at the start and returned Euclidean.  Same
 * arguments and workspace as pi3_bundle_adjust.  Restated from the published parametrization: parity unpinned. */
int pi3_bundle_adjust_inverse_depth(double* points, double* poses, const double* intr, const float* uv,
                                    const unsigned char* valid, const float* uvT, const unsigned char* validT, int N, int K,
                                    double huber_width, int max_iters, const double* prior_R, const double* prior_C,
                                    const unsigned char* prior_flag, double sqrt_info_rot, double sqrt_info_pos,
                                    double* summary_dev, double* workspace, long workspace_doubles, void* stream);

/* pt.sfm.SetOutlierTracksToUnestimated(tracks, max_reprojection_error_px, min_triangulation_angle_deg)
 * (utils/chunk_reconstruction.py:218, utils/reconstruction_alignment.py:170): estimated[s*K + k] = 1 iff every
 * observation of the track is in front of its camera and within max px, and two viewing rays subtend more than the
 * minimum angle. */
int pi3_ba_outlier_tracks(const double* points, const double* poses, const double* intr, const float* uv,
                          const unsigned char* valid, int N, int K, double max_reprojection_px,
                          double min_triangulation_angle_deg, unsigned char* estimated, void* stream);

/* ---- dense voxel map (csrc/voxel.hip): confidence-filtered fusion of the dense pointmaps into an open-addressing hash
 * table of voxels.  table: caller-owned DEVICE memory of 64 bytes per slot (key, W, U[3], C[3] as uint64), capacity a
 * power of two >= 2 x the candidate points fused since the last clear (the table never fills; no probe loop can run
 * for ever).  Integer accumulators only: results are bitwise reproducible whatever order the atomics land in.
 * Per point and axis (fp32, no contraction): s = p * inv_voxel, k = floor(s), u = min(trunc((s - k) * 2^24), 2^24 - 1);
 * the key packs k + 2^20 of x, y, z at 21 bits each (x << 42 | y << 21 | z).  Points that are not finite or have
 * |k| >= 2^20 are dropped and counted.  stats: DEVICE uint64 [4] = dropped, table overflows (0 under the capacity
 * rule), voxels written by the last extract, voxels the last extract could not store.
 * pi3_voxel_clear: every slot empty, stats zeroed. */
int pi3_voxel_clear(void* table, long capacity, unsigned long long* stats, void* stream);
/* One chunk's maps: points f32 [N][H][W][3], conf f32 logits [N][H][W] (or NULL), masks uint8 [N][H][W] (or NULL), imgs
 * f32 [N][3][H][W] in [0, 1] (or NULL: black).  A pixel counts when mask != 0 and conf > conf_logit_thr; weight 1;
 * colour = the keypoint colour rule, uint8 truncation of 255 c (saturated).  capacity >= 2 N H W. */
int pi3_voxel_fuse_pixels(void* table, long capacity, const float* points, const float* conf, const unsigned char* masks,
                          const float* imgs, int N, int H, int W, float conf_logit_thr, float inv_voxel,
                          unsigned long long* stats, void* stream);
/* A point list: points f32 [n][3], colors uint8 [n][3] (or NULL), weights int32 [n] (or NULL = 1; w <= 0 skips the
 * point).  Each point adds w, w u and w rgb to its voxel.  capacity >= 2 n. */
int pi3_voxel_fuse_points(void* table, long capacity, const float* points, const unsigned char* colors,
                          const int* weights, long n, float inv_voxel, unsigned long long* stats, void* stream);
/* Move every occupied slot of src into dst (a larger, cleared table): growth without losing the integer sums. */
int pi3_voxel_rehash(const void* src_table, long src_capacity, void* dst_table, long dst_capacity,
                     unsigned long long* stats, void* stream);
/* Every occupied slot -> keys uint64 [V], centroid f32 [V][3] = voxel_size (k + U / (W 2^24)) (f64 arithmetic),
 * colors uint8 [V][3] = (C + W / 2) / W, weights int32 [V] = min(W, 2^31 - 1), at most max_out entries; V lands in stats[2].  The order
 * of the entries is not defined (sort by key on the host). */
int pi3_voxel_extract(const void* table, long capacity, double voxel_size, unsigned long long* keys, float* points,
                      unsigned char* colors, int* weights, long max_out, unsigned long long* stats, void* stream);

/* pi3_voxel_extract for the occupied slots with keep[slot] != 0 only (keep: uint8 [capacity], see below); the rows
 * are computed exactly alike. */
int pi3_voxel_extract_kept(const void* table, long capacity, double voxel_size, unsigned long long* keys, float* points,
                           unsigned char* colors, int* weights, long max_out, unsigned long long* stats,
                           const unsigned char* keep, void* stream);

/* ---- cleaning the fused map (csrc/voxel_clean.hip): a keep / drop decision per slot of a voxel table, integer
 * arithmetic only.  The table is read only.  All arrays are caller-owned DEVICE memory with one entry per slot.
 *   eligible: an occupied slot with W >= min_weight;
 *   support(v): the eligible voxels u != v with max(|dx|, |dy|, |dz|) <= radius in voxel indices, radius 1 or 2; a
 *   cell whose index on an axis leaves |k| < 2^20 does not exist (nothing wraps into a neighbouring field);
 *   stage A survivors: eligible and support >= min_support (0 <= min_support <= (2 radius + 1)^3 - 1);
 *   stage B: 26-connected components of the survivors, label = the smallest key, size = the voxel count; kept: size >=
 *   min_component.  One pass of each, in this order.
 * counters: DEVICE uint64 [8] = occupied slots, eligible, after support, after components, components found,
 * components kept, 2 spare.
 * pi3_voxel_support: zeroes counters, writes keep uint8 [capacity] (1 = stage-A survivor, else 0), support int32
 * [capacity] (or NULL; -1 for a slot that is not eligible) and counters[0..2].  With min_support == 0 and support ==
 * NULL no neighbour is probed. */
int pi3_voxel_support(const void* table, long capacity, unsigned long long min_weight, int radius, int min_support,
                      unsigned char* keep, int* support, unsigned long long* counters, void* stream);
/* pi3_voxel_support with an exclude mask (uint8 [capacity]; the carved voxels of pi3_voxel_carve): an occupied slot
 * with exclude[slot] != 0 is not eligible (keep 0, support -1) and is not counted as anybody's neighbour, so the
 * components that follow are formed without it.  Everything else as above; also writes counters[6] = the occupied
 * slots that exclude names (counters[0] still counts every occupied slot). */
int pi3_voxel_support_excluding(const void* table, long capacity, unsigned long long min_weight, int radius,
                                int min_support, unsigned char* keep, int* support, unsigned long long* counters,
                                const unsigned char* exclude, void* stream);
/* label uint64 [capacity] = the slot's key where keep != 0, all ones elsewhere. */
int pi3_voxel_label_init(const void* table, long capacity, const unsigned char* keep, unsigned long long* label,
                         void* stream);
/* One labelling sweep: every survivor takes the minimum of its own and its 26 neighbours' labels, follows label[slot of
 * m] a bounded number of hops, and atomicMins a smaller m into its own label and into its previous root's; *changed (a
 * DEVICE int the caller zeroed) becomes 1 when a label was lowered.  Labels only decrease and always name a survivor of
 * the same component; the caller repeats the sweep until one leaves *changed at 0: then every label is its component's
 * smallest key, whatever order the atomics landed in.  At most (survivors) sweeps change anything. */
int pi3_voxel_label_sweep(const void* table, long capacity, unsigned long long* label, int* changed, void* stream);
/* size uint32 [capacity]: zeroed, then size[slot of label] += 1 per survivor (the converged labels). */
int pi3_voxel_component_sizes(const void* table, long capacity, const unsigned long long* label, unsigned* size,
                              void* stream);
/* keep[slot] = 0 where the slot's component has size < min_component; writes counters[3..5]. */
int pi3_voxel_component_filter(const void* table, long capacity, const unsigned long long* label, const unsigned* size,
                               long min_component, unsigned char* keep, unsigned long long* counters, void* stream);

/* ---- multi-view depth consistency of one chunk's dense maps (csrc/dense_filter.hip): a pixel mask for
 * pi3_voxel_fuse_pixels.  points f32 [N][H][W][3] (world), local_points f32 [N][H][W][3] (z = [..][2]), conf f32 logits
 * [N][H][W] (or NULL), masks uint8 [N][H][W] (or NULL), poses f32 [N][4][4] cam->world row-major, fxfycxcy f32 [N][4].
 * fp32, no contraction, every product and sum rounded on its own in the order written.
 *   candidate: mask != 0, conf > conf_logit_thr, the three world coordinates finite, local z finite and > 0;
 *   zplane (workspace f32 [N][H][W]) = local z of a candidate, else 0;
 *   per candidate of frame i and neighbour j = i +- s stride (s = 1..radius, j in [0, N)), R, t = poses[j]:
 *     d = X - t;  xc = (R00 dx + R10 dy) + R20 dz, yc and zc from columns 1 and 2;  no vote unless zc > 0 and all finite;
 *     u = fx (xc / zc) + cx, v = fy (yc / zc) + cy;  pu = rintf(u), pv = rintf(v);  no vote unless 0 <= pu <= W - 1 and
 *     0 <= pv <= H - 1;  zo = zplane[j][pv][pu], no vote when 0;  r = zc - zo, lim = rel_tol zo;
 *     agree when |r| <= lim, conflict when r < -lim (view j saw through the point), else occluded: no vote;
 *   out_mask uint8 [N][H][W] = agree >= min_views && conflict <= agree (0 for a non-candidate);
 *   counts uint8 [N][H][W][2] = agree, conflict, saturated at 255 (or NULL);  stats: DEVICE uint64 [2] = candidates,
 *   kept; zeroed by the call.
 * radius in 1..16, stride >= 1, min_views in 1..2 radius, rel_tol finite and > 0, N H W < 2^31.  N == 0 zeroes stats
 * and launches no kernel. */
int pi3_dense_consistency(const float* points, const float* local_points, const float* conf, const unsigned char* masks,
                          const float* poses, const float* fxfycxcy, int N, int H, int W, float conf_logit_thr,
                          int radius, int stride, int min_views, float rel_tol, float* zplane, unsigned char* out_mask,
                          unsigned char* counts, unsigned long long* stats, void* stream);

/* Depth keyframes of one chunk (csrc/dense_filter.hip), for pi3_voxel_carve: for the frames f = 0, every, 2 every, .. < N
 * (Nk = ceil(N / every) of them) and the pixels (S y', S x') with S = pixel_stride in {1, 2, 4}, H' = ceil(H / S),
 * W' = ceil(W / S):  depth[k][y'][x'] (fp16 bits, uint16 [Nk][H'][W']) = the local z of frame k every at that pixel,
 * rounded to nearest even, when the pixel is a candidate of pi3_dense_consistency (mask != 0, conf > conf_logit_thr,
 * world point finite, local z finite and > 0), else 0; a value that rounds to 0 or to inf is written as 0 ("this view
 * has no opinion here").  *count (DEVICE uint64, zeroed by the call) = the non-zero samples.  conf and masks may be
 * NULL.  N H W < 2^31; N == 0 zeroes the count and launches no kernel. */
int pi3_dense_depth_planes(const float* points, const float* local_points, const float* conf, const unsigned char* masks,
                           int N, int H, int W, float conf_logit_thr, int every, int pixel_stride,
                           unsigned short* depth, unsigned long long* count, void* stream);

/* ---- carving the fused map with depth keyframes (csrc/voxel_carve.hip): one decision per slot of a voxel table, f64
 * without contraction, every product and sum rounded on its own in the order written.  The table is read only.
 *   X = the centroid pi3_voxel_extract writes for the slot: voxel_size (k + U / (W 2^24)) in f64, rounded to fp32 and
 *   widened again;
 *   views f64 [M][20] in pi3_render_splat's camera layout (rigid world->camera 3x4 row-major r00 r01 r02 t0 .., fx, fy,
 *   cx, cy, ortho flag = 0, 3 spare) with views[m][17] = s, the depth scale of view m (its plane's unit in map units);
 *   planes fp16 bits [M][Hp][Wp] (pi3_dense_depth_planes), plane m for view m, S = pixel_stride in {1, 2, 4};
 *   per view:  xc = ((r00 x + r01 y) + r02 z) + t0, likewise yc, zc;  no vote unless zc > 0 and all three finite;
 *     u = fx (xc / zc) + cx, v = fy (yc / zc) + cy;  pu = rint(u / S), pv = rint(v / S) (half to even);  no vote unless
 *     0 <= pu <= Wp - 1 and 0 <= pv <= Hp - 1;  zo = s (double)plane[pv][pu];  no vote when zo is 0 or not finite;
 *     r = zc - zo, lim = rel_tol zo + margin;  agree when |r| <= lim, conflict when r < -lim (the view measured a
 *     surface behind the voxel: it looked through it), else occluded: no vote;
 *   carved uint8 [capacity] = conflict >= min_conflicts && conflict > agree (0 for an empty slot);
 *   agree, conflict uint32 [capacity] (or NULL): the votes, not saturated;
 *   counters: DEVICE uint64 [4] = occupied slots, carved, occupied slots no view voted on, spare; zeroed by the call.
 * rel_tol finite and > 0, margin finite and >= 0, min_conflicts >= 1, M >= 0 (0: nothing is carved). */
int pi3_voxel_carve(const void* table, long capacity, double voxel_size, const double* views, int M,
                    const unsigned short* planes, int Hp, int Wp, int pixel_stride, double rel_tol, double margin,
                    int min_conflicts, unsigned char* carved, unsigned* agree, unsigned* conflict,
                    unsigned long long* counters, void* stream);

/* ---- moving a chunk's dense cloud with the views that saw it (csrc/cloud_follow.hip): one blend of per-view moves per
 * point, f64 without contraction, every product and sum rounded on its own in the order written.
 *   points f32 [P][3], normals f32 [P][3] or NULL;  views f64 [M][20] in pi3_voxel_carve's layout (rigid frame->camera
 *   3x4 row-major, fx, fy, cx, cy, 0, views[m][17] = the unit of plane m in the points' units);  moves f64 [M][12]: D_m,
 *   3x4 row-major;  planes fp16 bits [M][Hp][Wp] (pi3_dense_depth_planes), S = pixel_stride in {1, 2, 4}.
 *   Per point X = (x, y, z) widened to f64.  X not finite: the outputs are the inputs, level 0, support 0, counters[0].
 *   Else for m = 0 .. M-1 in order, d = moves[m]:
 *     Y = (((d0 x + d1 y) + d2 z) + d3, ((d4 x + d5 y) + d6 z) + d7, ((d8 x + d9 y) + d10 z) + d11);
 *     Nn = ((d0 nx + d1 ny) + d2 nz, (d4 nx + d5 ny) + d6 nz, (d8 nx + d9 ny) + d10 nz);
 *     level 3 takes every view:  S3 += Y, N3 += Nn;
 *     xc, yc, zc, u, v, pu, pv as pi3_voxel_carve forms them;  next view unless zc > 0, xc yc zc finite and
 *     0 <= pu <= Wp - 1, 0 <= pv <= Hp - 1;
 *     w = 1.0 / (zc zc);  level 2:  S2 += w Y, W2 += w, N2 += w Nn, ++n2;
 *     zo = views[m][17] (double)plane[m][pv][pu];  next view when zo is 0 or not finite;
 *     |zc - zo| <= rel_tol zo + margin:  level 1:  S1 += w Y, W1 += w, N1 += w Nn, ++n1;
 *   level uint8 [P] (or NULL) = 1 when n1 > 0, else 2 when n2 > 0, else 3;  support int32 [P] (or NULL) = n1;
 *   out_points f32 [P][3] = S_l / W_l per component (level 3: S3 / (double)M);  out_normals f32 [P][3] = N_l /
 *   sqrt((Nx Nx + Ny Ny) + Nz Nz) when that sum is positive and finite, else 0.  out_points may be points, out_normals
 *   may be normals; normals and out_normals are both given or both NULL.
 *   counters: DEVICE uint64 [4] = points not finite, points of level 1, 2, 3; zeroed by the call.
 * M >= 1, rel_tol finite and > 0, margin finite and >= 0, 0 <= P < 2^39.  P == 0 zeroes the counters and launches no
 * kernel; points and out_points may then be NULL. */
int pi3_cloud_follow_views(const float* points, const float* normals, long P, const double* views, const double* moves,
                           int M, const unsigned short* planes, int Hp, int Wp, int pixel_stride, double rel_tol,
                           double margin, float* out_points, float* out_normals, unsigned char* level, int* support,
                           unsigned long long* counters, void* stream);

/* ---- occupancy grid and clearance field of the dense map (csrc/occupancy.hip).  A grid of cells of edge c with the
 * integer origin (ox, oy, oz) and the dimensions (nx, ny, nz): cell (ix, iy, iz) covers [c (o + i), c (o + i + 1)) per
 * axis and lies at the linear index (iz ny + iy) nx + ix (x fastest).  state uint8 [nz][ny][nx]: 0 unknown, 1 free,
 * 2 occupied.  |o| < 2^21 and 1 <= n < 2^21 per axis.
 * pi3_occupancy_mark: zeroes the grid, then per row of points f32 [P][3] (the extracted map): every axis through the
 *   voxel quantiser at inv_cell = (float)(1 / c) (k = floor(p * inv_cell) in fp32; dropped when not finite or
 *   |k| >= 2^20), i = k - o, state = 2 when the cell is inside the grid.  counters: DEVICE uint64 [4] = points marked,
 *   points dropped by the quantiser, points outside the grid, spare; zeroed by the call.  0 <= P < 2^39; P == 0 leaves
 *   an all-unknown grid.
 * pi3_occupancy_observe: per cell that is not occupied (state != 2; an occupied cell keeps its byte), the centre
 *   X = c ((double)(o + i) + 0.5) per axis, f64, and per view m in order pi3_voxel_carve's arithmetic, operation for
 *   operation (views f64 [M][20] with views[m][17] the depth scale, planes fp16 bits [M][Hp][Wp], S = pixel_stride):
 *   xc, yc, zc, u, v, pu, pv, zo and the same "no vote" cases;  r = zc - zo, lim = rel_tol zo + margin;  r < -lim is a
 *   free vote (the view measured a surface behind the centre), |r| <= lim a hit vote;
 *   state = 1 when free >= min_free_views && free > hit, else 0.
 *   Then, for the views in order, the cell a camera stands in: centre_j = -((r0j t0 + r1j t1) + r2j t2),
 *   k = floor(centre / c) per axis in f64; when that cell lies inside the grid and is unknown it becomes free (a view
 *   cannot look through its own position, but a camera stood there).  The votes are left as they are.
 *   free_votes, hit_votes uint32 [cells] (or NULL): the votes, 0 for an occupied cell;
 *   counters: DEVICE uint64 [8] = cells, occupied, free, unknown, cells that are not occupied and no view voted on,
 *   the unknown cells a camera's position made free (counted in free, not in unknown), 2 spare; zeroed by the call.  rel_tol finite and > 0, margin finite and >= 0, min_free_views >= 1, M >= 0 (0: no
 *   cell is free), at most 2^39 cells.
 * pi3_grid_edt: the exact squared Euclidean distance transform in cells, truncated at radius R in 1..255.  Sites are the
 *   cells with state == 2 and, when unknown_is_obstacle != 0, those with state == 0.  d2 uint16 [cells] = the squared
 *   distance to the nearest site when it is <= R^2, else 0xFFFF.  Three separable passes (x, y, z), each
 *   out[i] = min over |d| <= R of in[i + d] + d^2 in integers with values above R^2 clamped to 0xFFFF; the passes
 *   ping-pong between d2 and workspace (uint16 [cells], caller-owned, not d2), never in place.
 * Bad arguments launch nothing and leave the outputs untouched.  No allocation, no synchronisation. */
int pi3_occupancy_mark(const float* points, long P, float inv_cell, int ox, int oy, int oz, int nx, int ny, int nz,
                       unsigned char* state, unsigned long long* counters, void* stream);
int pi3_occupancy_observe(unsigned char* state, int nx, int ny, int nz, int ox, int oy, int oz, double cell,
                          const double* views, int M, const unsigned short* planes, int Hp, int Wp, int pixel_stride,
                          double rel_tol, double margin, int min_free_views, unsigned* free_votes, unsigned* hit_votes,
                          unsigned long long* counters, void* stream);
int pi3_grid_edt(const unsigned char* state, int nx, int ny, int nz, int radius, int unknown_is_obstacle,
                 unsigned short* d2, unsigned short* workspace, void* stream);

/* ---- routes through the occupancy grid (csrc/grid_route.hip): the same grid layout; integers only.  walk uint8 [cells]:
 * 1 = traversable.  The graph: the 26 moves d in {-1, 0, 1}^3 \ {0} at the costs 12, 17, 21 for one, two, three non-zero
 * components; a move c -> c + d is allowed only when every cell c + (a dx, b dy, e dz), a, b, e in {0, 1}, lies inside the
 * grid and is traversable (no corner is cut; the rule is symmetric).  dist uint32 [cells]: the cheapest move sequence
 * from any source, 0xFFFFFFFF when there is none.  1 <= n < 2^21 per axis and at most 2^27 cells, so that 21 (cells - 1)
 * stays below the far mark.
 * pi3_grid_route_init: walk = (state == 1; with through_unknown != 0: state != 2) and, when d2 is given (pi3_grid_edt's
 *   field, uint16 [cells]), d2 >= min_d2 (0 .. 65 025; the field's far mark 0xFFFF passes; min_d2 > 0 needs d2).
 *   dist = 0xFFFFFFFF everywhere, then 0 at every source: sources int64 [Ns] are linear indices; one outside [0, cells)
 *   or on a cell that is not traversable is only counted.  counters: DEVICE uint64 [4] = traversable cells, sources
 *   accepted (a duplicate counts again), sources not traversable, sources outside; zeroed by the call.  0 <= Ns < 2^39;
 *   Ns == 0 leaves an all-far field and sources may be NULL.
 * pi3_grid_route_sweep: one relaxation sweep, a workgroup per tile of 8 x 8 x 8 cells: the tile's cells are relaxed to
 *   their fixed point against each other and against the tile's one-cell halo as it is read; cells that got lower are
 *   stored, and *changed (DEVICE int32, never cleared here) becomes 1 when any did.  The caller repeats the call until a
 *   sweep leaves its `changed` word 0: dist is then the shortest-distance field, whatever order the tiles ran in (values
 *   are costs of real move sequences, only decrease, and 32-bit words do not tear).
 * pi3_grid_route_trace: one wave walks from `goal` (a linear index) back to a source over a settled dist: at every cell
 *   the neighbour n with an allowed move and dist[n] + w == dist[cur] that has the smallest linear index.  path int64
 *   [cap]: the linear indices from the goal to the source; *length (DEVICE int64) = their number, 0 when the goal is not
 *   traversable or not reachable (or dist is not settled), -needed when cap is too small: path is then left untouched.
 *   cap = dist[goal] / 12 + 1 always suffices.
 * Bad arguments launch nothing and leave the outputs untouched.  No allocation, no synchronisation. */
int pi3_grid_route_init(const unsigned char* state, const unsigned short* d2, int min_d2, int through_unknown, int nx,
                        int ny, int nz, const long* sources, long Ns, unsigned char* walk, unsigned* dist,
                        unsigned long long* counters, void* stream);
int pi3_grid_route_sweep(const unsigned char* walk, int nx, int ny, int nz, unsigned* dist, int* changed, void* stream);
int pi3_grid_route_trace(const unsigned char* walk, const unsigned* dist, int nx, int ny, int nz, long goal, long* path,
                         long cap, long* length, void* stream);
/* Several fields over one walk: dist uint32 [K][cells], field f the distances from sources[f] alone;
 * 1 <= K <= 65 535.
 * pi3_grid_route_fields_init: every field = 0xFFFFFFFF everywhere, then field f gets 0 at sources[f] (DEVICE int64 [K],
 *   linear indices) when that index lies inside [0, cells) on a traversable cell; a field whose source is refused stays
 *   all far.  counters: DEVICE uint64 [3] = sources accepted, not traversable, outside; zeroed by the call.
 * pi3_grid_route_sweep_many: one pi3_grid_route_sweep of every field listed in active (DEVICE int32 [A], distinct field
 *   numbers in 0 .. K - 1; an entry outside that range is passed over), a workgroup per tile and `group` listed fields:
 *   the tile's walk bytes are staged once, then field after field.  changed: DEVICE int32 [K], never cleared here;
 *   changed[f] becomes 1 when a cell of field f got lower.  Fields that are not listed are neither read nor written, and
 *   neither are their entries of changed.  The fixed point of every field is pi3_grid_route_sweep's.  0 <= A <= K; A == 0
 *   launches nothing and active may be NULL.  group >= 1 (more than A means A).
 * pi3_grid_route_trace_many: one wave per leg l < L walks by pi3_grid_route_trace's rules over field field_of[l] from
 *   goal[l] into path[offset[l] .. offset[l + 1]): field_of DEVICE int32 [L], goal DEVICE int64 [L], offset DEVICE int64
 *   [L + 1] ascending, length DEVICE int64 [L]; length[l] = the waypoints, 0 when there is no way (or field_of[l] or
 *   goal[l] is out of range), -needed when the slot is too short: the slot is then left untouched.  L >= 0; L == 0
 *   launches nothing and the per-leg arrays may be NULL.
 * Bad arguments launch nothing and leave the outputs untouched.  No allocation, no synchronisation. */
int pi3_grid_route_fields_init(const unsigned char* walk, int nx, int ny, int nz, const long* sources, int K,
                               unsigned* dist, unsigned long long* counters, void* stream);
int pi3_grid_route_sweep_many(const unsigned char* walk, int nx, int ny, int nz, unsigned* dist, int K,
                              const int* active, int A, int group, int* changed, void* stream);
int pi3_grid_route_trace_many(const unsigned char* walk, const unsigned* dist, int nx, int ny, int nz, int K,
                              const int* field_of, const long* goal, const long* offset, long* path, long* length, int L,
                              void* stream);
/* Line of sight over the same walk (csrc/grid_sight.hip).  Cell a SEES cell b when every cell whose closed
 * cube meets the segment between the two centres is traversable (the closed supercover: where the segment runs through
 * an edge or a corner of the lattice, all 4 or 8 cells around it are touched).  Exact in 32-bit integers for two cells
 * of a grid of at most 2^27 cells; symmetric; for two neighbours it is the move rule above.
 * pi3_grid_route_sight_paths: the cells of `legs` ways one after the other, way l = cells[offsets[l] .. offsets[l + 1])
 *   (cells DEVICE int64 [P] linear indices, offsets DEVICE int64 [legs + 1] ascending from 0 to P).  vis: DEVICE uint64
 *   [P][ceil(span / 64)]; bit k of row p is set when p and p + 1 + k lie in the same way, k < span, and cells[p] sees
 *   cells[p + 1 + k]; every other bit of every word is written 0.  An index outside [0, cells) sees nothing.
 *   0 <= P < 2^31, legs >= 0, 1 <= span <= 4096; P == 0 or legs == 0 launches nothing and the arrays may be NULL.
 * pi3_grid_route_sight_pairs: N arbitrary pairs a[i], b[i] (DEVICE int64 [N]).  The whole segment is walked even after
 *   a blocked cell: sees uint8 [N] = 1 / 0, touched int32 [N] = the cells of the supercover, min_d2 uint16 [N] = the
 *   smallest d2 (pi3_grid_edt's field, uint16 [cells]) over them, 0xFFFF when d2 is NULL.  An end outside [0, cells)
 *   gives 0, 0, 0xFFFF.  0 <= N < 2^39; N == 0 launches nothing and the arrays may be NULL.
 * Bad arguments launch nothing and leave the outputs untouched.  No allocation, no synchronisation. */
int pi3_grid_route_sight_paths(const unsigned char* walk, int nx, int ny, int nz, const long* cells, long P,
                               const long* offsets, int legs, int span, unsigned long long* vis, void* stream);
int pi3_grid_route_sight_pairs(const unsigned char* walk, const unsigned short* d2, int nx, int ny, int nz, const long* a,
                               const long* b, long N, unsigned char* sees, int* touched, unsigned short* min_d2,
                               void* stream);

/* ---- frontiers of the occupancy grid (csrc/grid_frontier.hip): the same grid layout and limits (1 <= n < 2^21 per
 * axis, at most 2^27 cells); integers only.  A frontier cell is a cell with state == 1 of whose 6 face neighbours at
 * least one is unknown (state == 0); a neighbour outside the grid counts as unknown (the box only bounds where points
 * and cameras were: nothing beyond it was ever voted on).  label uint32 [cells]: 0xFFFFFFFF for a cell that is no
 * frontier cell.
 * pi3_grid_frontier_mark: label[c] = c for a frontier cell, else 0xFFFFFFFF.  counters: DEVICE uint64 [4] = frontier
 *   cells, unknown faces over all frontier cells (1..6 each), 2 spare; zeroed by the call.
 * pi3_grid_frontier_sweep: one sweep of minimum-label propagation over plain 26-connectivity among the labelled cells
 *   (no corner rule), a workgroup per tile of 8 x 8 x 8 cells: the tile's cells are relaxed to their fixed point against
 *   each other and against the tile's one-cell halo as it is read; cells that got lower are stored, and *changed
 *   (DEVICE int32, never cleared here) becomes 1 when any did.  A tile without a labelled cell writes nothing.  The
 *   caller repeats the call until a sweep leaves its `changed` word 0: every labelled cell then carries the smallest
 *   linear index of its component, whatever order the tiles ran in (values are indices of cells of the same component,
 *   only decrease, and 32-bit words do not tear).
 * pi3_grid_frontier_roots: the cells with label[c] == c, compacted in any order into roots int64 [cap]; *count (DEVICE
 *   int64, zeroed by the call) = their number even when it exceeds cap: the first cap slots claimed are then written and
 *   the caller must check.  cap >= 0; roots may be NULL at cap == 0.
 * pi3_grid_frontier_stats: roots_sorted int64 [K] ascending (pi3_grid_frontier_roots' output, sorted by the host).  The
 *   call initialises stats int64 [K][12] and every frontier cell (label != 0xFFFFFFFF) reduces into the row whose root is
 *   its label: cells, unknown faces, the sums of x, y, z, the minima of x, y, z (initially INT64_MAX), the maxima of x,
 *   y, z (initially -1), and `best`, as uint64 the smallest (dist[c] << 27) | c over the cells with dist[c] !=
 *   0xFFFFFFFF: the cheapest reachable cell and, among equals, the smallest index; all ones when there is none or dist
 *   (uint32 [cells], pi3_grid_route_sweep's settled field) is NULL.  Integer atomics: the bytes do not depend on the
 *   order.  counters: DEVICE uint64 [4] = cells reduced, cells whose label is not in roots_sorted (0 from a correct
 *   caller; they are reduced nowhere), cells with a finite dist, 1 spare; zeroed by the call.  0 <= K <= cells; K == 0
 *   zeroes the counters and launches no kernel, roots_sorted and stats may then be NULL.
 * Bad arguments launch nothing and leave the outputs untouched.  No allocation, no synchronisation. */
int pi3_grid_frontier_mark(const unsigned char* state, int nx, int ny, int nz, unsigned* label,
                           unsigned long long* counters, void* stream);
int pi3_grid_frontier_sweep(int nx, int ny, int nz, unsigned* label, int* changed, void* stream);
int pi3_grid_frontier_roots(const unsigned* label, int nx, int ny, int nz, long* roots, long cap, long* count,
                            void* stream);
int pi3_grid_frontier_stats(const unsigned char* state, const unsigned* label, const unsigned* dist, int nx, int ny,
                            int nz, const long* roots_sorted, long K, long* stats, unsigned long long* counters,
                            void* stream);

/* ---- views of the occupancy grid (csrc/grid_view.hip): the same grid layout and limits; integers only.  Cell m lies
 * between cells v and u when the open segment between their centres meets m's open interior (v and u never count; a
 * cell the segment only touches at a face, edge or corner does not either): the integer DDA from v along o = u - v with
 * the k-th crossing of axis a at t = (2k - 1) / (2 |o_a|), always the smallest t, all axes tied at that t stepping at
 * once.  u is visible from v when no cell between them is occupied (state == 2); unknown and free cells are
 * transparent.  A target of candidate v at range R is a cell u != v inside the grid with |u - v|^2 <= R^2 and
 * state[u] == 0.  Offset o lies in the cone of heading a when o.a > 0 and (o.a)^2 den >= num |o|^2 |a|^2 (64 bits;
 * num / den = cos^2 of half the field of view; the boundary is inside).
 * pi3_grid_view_candidates: the cells of dist uint32 [cells] (pi3_grid_route_sweep's settled field) with dist !=
 *   0xFFFFFFFF, dist <= max_cost (>= 0) and the ABSOLUTE index (ox + x, oy + y, oz + z) a multiple of stride (>= 1) on
 *   every axis (floor modulo: the origin may be negative), compacted in any order into cells int64 [cap]; *count (DEVICE
 *   int64, zeroed by the call) = their number even when it exceeds cap: the first cap slots claimed are then written and
 *   the caller must check.  cap >= 0; cells may be NULL at cap == 0.
 * pi3_grid_view_gain: candidates int64 [V] are linear indices, on cells of any state.  headings: HOST int [H][3], 1 <= H
 *   <= 32, every axis non-zero with components within +-1024 (read during the call and passed to the kernel by value).
 *   range in 1..32 cells; 0 <= num <= den, 0 < den < 2^31.  Per candidate: visible[v] = the visible targets, gain[v][h]
 *   (uint32 [V][H]) = those in heading h's cone, best[v] = the smallest h of the largest gain.  A candidate outside
 *   [0, cells) gets zeros and best = -1 and is not counted.  counters: DEVICE uint64 [4] = candidates inside the grid,
 *   targets (rays cast), rays blocked, rays visible; zeroed by the call.  0 <= V < 2^31; V == 0 zeroes the counters and
 *   launches no kernel, the per-candidate arrays may then be NULL.  Integer sums only: the bytes do not depend on the
 *   order.
 * Bad arguments launch nothing and leave the outputs untouched.  No allocation, no synchronisation. */
int pi3_grid_view_candidates(const unsigned* dist, int nx, int ny, int nz, int ox, int oy, int oz, int stride,
                             long max_cost, long* cells, long cap, long* count, void* stream);
int pi3_grid_view_gain(const unsigned char* state, int nx, int ny, int nz, const long* candidates, long V, int range,
                       const int* headings, int H, long cos2_num, long cos2_den, unsigned* gain, unsigned* visible,
                       int* best, unsigned long long* counters, void* stream);
/* Views that cover: a mask of the cells that kept views already see.  seen: DEVICE uint32
 * [(cells + 31) >> 5], cell c (the linear index) is bit c & 31 of word c >> 5; bits at positions >= cells are never set.
 * pi3_grid_view_gain_unseen: pi3_grid_view_gain with one more condition on a target: its bit of seen is clear.  Every
 *   output and counter keeps its meaning, counted over those targets; with an all-zero mask the bytes are
 *   pi3_grid_view_gain's.  seen is read only and must not be NULL.
 * pi3_grid_view_mark: row i is the view (cells[i], heading_of[i]): cells DEVICE int64 [V], heading_of HOST int [V] with
 *   every entry in -1 .. H - 1 (read and checked during the call and passed to the kernel by value: one launch when all
 *   rows share a heading, else 1024 rows per launch).
 *   A ray is cast to every target of the cell (the mask is ignored here); the bit of every target that is visible and in
 *   heading_of[i]'s cone (-1: in the cone of at least one of the H headings) is set, by an atomic OR that is issued only
 *   when the bit read clear.  owner: DEVICE int16 [cells] or NULL; the lane that turned a bit from 0 to 1 writes
 *   owner[u] = tag, 0 <= tag < 32768; with an owner V must be 1 (rows racing for a cell would not be reproducible).
 *   counters: DEVICE uint64 [5] = views (rows inside the grid), rays cast, rays visible, visible and in the cone, new
 *   bits; zeroed by the call.  A cell outside [0, cells) marks nothing and is no view.  V == 0 zeroes the counters and
 *   launches no kernel; cells and heading_of may then be NULL.  range, headings, H, num, den as pi3_grid_view_gain.
 * Bad arguments launch nothing and leave the outputs untouched.  No allocation, no synchronisation. */
int pi3_grid_view_gain_unseen(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                              const long* candidates, long V, int range, const int* headings, int H, long cos2_num,
                              long cos2_den, unsigned* gain, unsigned* visible, int* best, unsigned long long* counters,
                              void* stream);
int pi3_grid_view_mark(const unsigned char* state, int nx, int ny, int nz, unsigned* seen, const long* cells,
                       const int* heading_of, long V, int range, const int* headings, int H, long cos2_num,
                       long cos2_den, short* owner, int tag, unsigned long long* counters, void* stream);
/* Views that see farther (csrc/grid_view.hip): the three ray entry points with range in 1..64.  Every
 * argument, rule, output and counter is its namesake's, and for range <= 32 so is every byte.  A workgroup takes one
 * octant of a pose (a ray never leaves the closed octant of its target; a target o belongs to the octant that is
 * positive on axis a when o_a >= 0) and adds its counts to gain, visible and the counters with integer atomics, which
 * the call zeroes first on the stream; best is written by a finishing kernel.  One more argument check: the cone
 * test's (o.a)^2 den is formed in 64 bits, so a call with range^2 * max_h |a_h|^2 * den >= 2^63 is refused (|a|^2 <= 3
 * and den = 2^20 are far inside).  Bad arguments launch nothing and leave the outputs untouched.  No allocation, no
 * synchronisation. */
int pi3_grid_view_gain_far(const unsigned char* state, int nx, int ny, int nz, const long* candidates, long V, int range,
                           const int* headings, int H, long cos2_num, long cos2_den, unsigned* gain, unsigned* visible,
                           int* best, unsigned long long* counters, void* stream);
int pi3_grid_view_gain_unseen_far(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                                  const long* candidates, long V, int range, const int* headings, int H, long cos2_num,
                                  long cos2_den, unsigned* gain, unsigned* visible, int* best,
                                  unsigned long long* counters, void* stream);
int pi3_grid_view_mark_far(const unsigned char* state, int nx, int ny, int nz, unsigned* seen, const long* cells,
                           const int* heading_of, long V, int range, const int* headings, int H, long cos2_num,
                           long cos2_den, short* owner, int tag, unsigned long long* counters, void* stream);
/* Unknown space that ends a ray (csrc/grid_view.hip): the ray entry points with one more rule.  u is
 * visible from v at depth K when no cell between them is occupied and at most K cells between them are unknown;
 * "between" is the rule above, so v, u and the target's own state never count.  depth is 0..255; a ray of the ball of
 * 64 cells has at most 109 cells between its ends, so depth >= 110 gives the bytes of the entry points above.  far: 0
 * for the whole box (range 1..32), 1 for the octant form (range 1..64, with the far form's check of the cone).  seen
 * of pi3_grid_view_gain_depth may be NULL: every unknown cell is then a target (pi3_grid_view_gain), else only those
 * whose bit is clear (pi3_grid_view_gain_unseen).  Every other argument, output and counter is its namesake's;
 * "blocked" counts every ray that did not arrive, whichever rule ended it.  Bad arguments return PI3_ERR_ARG with the
 * depth's bounds in the message and launch nothing; V == 0 launches no kernel.  The first launch per device whose box
 * needs more than 64 KB of LDS (near range 32, far range 63 and 64) sets the kernel's LDS limit once. */
int pi3_grid_view_gain_depth(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                             const long* candidates, long V, int range, int depth, int far, const int* headings, int H,
                             long cos2_num, long cos2_den, unsigned* gain, unsigned* visible, int* best,
                             unsigned long long* counters, void* stream);
int pi3_grid_view_mark_depth(const unsigned char* state, int nx, int ny, int nz, unsigned* seen, const long* cells,
                             const int* heading_of, long V, int range, int depth, int far, const int* headings, int H,
                             long cos2_num, long cos2_den, short* owner, int tag, unsigned long long* counters,
                             void* stream);
/* Views through a camera (csrc/grid_view.hip): the ray entry points with a frustum per heading instead of
 * a cone.  frames: HOST int [H][6], 1 <= H <= 32, row h = f (forward) then r (right): both non-zero, f.r = 0, every
 * component within +-64 (read during the call and passed to the kernel by value); u = f x r.  Offset o = u_cell - v
 * lies in frame h's frustum when o.f > 0, (o.r)^2 |f|^2 hd <= hn (o.f)^2 |r|^2 and (o.u)^2 vd <= vn (o.f)^2 |r|^2, in
 * 64 bits, the faces inclusive: tan^2 of half the horizontal and the vertical field of view are hn / hd and vn / vd
 * with 0 <= num <= 2^20 and 1 <= den <= 2^20.  Only directions matter: a positive multiple of f or r, or -r, gives
 * the same bytes.  depth: -1 for transparent unknown space, else 0..255 as pi3_grid_view_gain_depth; far and seen
 * (NULL: every unknown cell is a target) as there.  Every other argument, output and counter is its namesake's, with
 * "in the cone" read as "in the frustum"; heading -1 of a mark row is "inside any frame's frustum".  Bad arguments
 * return PI3_ERR_ARG with every rule in the message and launch nothing; V == 0 launches no kernel.  The LDS opt-in is
 * the depth entry points'. */
int pi3_grid_view_gain_frustum(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                               const long* candidates, long V, int range, int depth, int far, const int* frames, int H,
                               long tan2_h_num, long tan2_h_den, long tan2_v_num, long tan2_v_den, unsigned* gain,
                               unsigned* visible, int* best, unsigned long long* counters, void* stream);
int pi3_grid_view_mark_frustum(const unsigned char* state, int nx, int ny, int nz, unsigned* seen, const long* cells,
                               const int* heading_of, long V, int range, int depth, int far, const int* frames, int H,
                               long tan2_h_num, long tan2_h_den, long tan2_v_num, long tan2_v_den, short* owner, int tag,
                               unsigned long long* counters, void* stream);

/* ---- routes for a body that stands (csrc/grid_stand.hip): the same grid layout and limits; integers only.
 * up = up_sign e_up_axis is one of the six signed axes (up_axis 0, 1, 2 = x, y, z; up_sign 1 or -1).  A cell is passable
 * when state == 1, with through_unknown != 0 when state != 2.
 * pi3_grid_stand_height: height uint8 [cells], whatever the cell's own state: look at c - j up for j = 1 .. 254 and stop
 *   at the first cell that is outside the grid or not passable.  Stopped on an occupied cell: j.  Stopped on an unknown
 *   cell or at the border: 0 (no verified support).  Never stopped: 255.  One pass that reads state along x for every
 *   direction and writes every byte once.
 * pi3_grid_route_init_stand: pi3_grid_route_init with one more condition, h_lo <= height <= h_hi (1 <= h_lo <= h_hi <=
 *   254).  counters: DEVICE uint64 [5], [0 .. 3] as there, [4] = the cells that pi3_grid_route_init's rule alone would
 *   have opened and the band closed; zeroed by the call.
 * pi3_grid_view_candidates_stand: pi3_grid_view_candidates with the lattice of a standing planner: on the two axes other
 *   than up_axis the absolute index is a multiple of stride, along up_axis (height - h_lo) mod stride == 0 (floor modulo;
 *   1 <= h_lo <= 254), so that every column that stands offers its lowest band cell whatever level its floor is at.
 * Bad arguments launch nothing and leave the outputs untouched.  No allocation, no synchronisation. */
int pi3_grid_stand_height(const unsigned char* state, int nx, int ny, int nz, int up_axis, int up_sign,
                          int through_unknown, unsigned char* height, void* stream);
int pi3_grid_route_init_stand(const unsigned char* state, const unsigned short* d2, int min_d2, int through_unknown,
                              const unsigned char* height, int h_lo, int h_hi, int nx, int ny, int nz,
                              const long* sources, long Ns, unsigned char* walk, unsigned* dist,
                              unsigned long long* counters, void* stream);
int pi3_grid_view_candidates_stand(const unsigned* dist, const unsigned char* height, int nx, int ny, int nz, int ox,
                                   int oy, int oz, int stride, long max_cost, int up_axis, int h_lo, long* cells,
                                   long cap, long* count, void* stream);

/* ---- nearest neighbours between two point clouds (csrc/cloud_nn.hip): an exact radius-bounded search through a
 * uniform grid of cells, for scoring a map against a reference cloud (map_eval.py).  The grid is a hash table of cells
 * in the voxel table's form: `capacity` slots of 64 B (a power of two, at least 2 n: ops.voxel_capacity), keyed by the
 * cell indices floor(fl(p * inv_cell)) per axis exactly as the voxel quantiser forms them (fp32 product, |k| < 2^20).
 *   slot = key | count | start | fill | row cursor (slot 0 only) | 3 spare, as uint64;
 *   cells: n rows of 16 B = x, y, z (f32 bits), the point's index in `points` (int32); the rows of one cell are
 *   cells[start .. start + count).  The order of the rows in a cell and of the cells in the array is not defined.
 * pi3_cloud_index_build: points f32 [n][3].  Clears the table, counts the points per cell, gives every occupied cell
 * its rows (one atomic add per workgroup on the cursor) and writes the rows.  A point that is not finite or whose cell
 * index has |k| >= 2^20 on an axis is dropped: counted, no row.  counters: DEVICE uint64 [4] = dropped points,
 * occupied cells, points that found no slot (0 under the capacity rule; they get no row), the largest cell's count;
 * zeroed by the call.  0 <= n < 2^31; n == 0 leaves an empty table and launches no pass; points and cells may then be
 * NULL.  inv_cell finite and > 0.  No allocation, no synchronisation. */
int pi3_cloud_index_build(const float* points, long n, float inv_cell, void* table, long capacity, void* cells,
                          unsigned long long* counters, void* stream);
/* pi3_cloud_nearest: table, cells, n and inv_cell as pi3_cloud_index_build left them; queries f32 [m][3].  A query visits
 * the 27 cells around its own (a cell whose index leaves |k| < 2^20 does not exist) and for every row p of them
 * computes, in f64 without contraction, every operation rounded on its own in this order:
 *   dx = (double)qx - (double)px, likewise dy, dz;   d2 = (dx dx + dy dy) + dz dz;
 *   a row is a candidate when d2 <= max_dist max_dist (inclusive; the product formed once in f64);
 *   d2[i] f64, idx[i] int32 = the candidate with the smallest d2 and, among equal d2, the smallest original index:
 *   independent of the row order, bitwise reproducible.  No candidate: d2 = +inf, idx = -1.  A query the quantiser
 *   drops is counted and gets +inf / -1.  NaN is written nowhere.
 * The result is the exact nearest neighbour within max_dist among the points the index holds when max_dist * inv_cell
 * <= 0.9 (callers use cells of 1.25 max_dist: 0.8); a larger product is refused.
 * counters: DEVICE uint64 [4] = dropped queries, matched, beyond (no candidate), distance evaluations; zeroed by the
 * call.  m == 0 launches nothing; n == 0: every query is beyond (none is dropped), cells may be NULL. */
int pi3_cloud_nearest(const void* table, long capacity, const void* cells, long n, float inv_cell, const float* queries,
                      long m, double max_dist, double* d2, int* idx, unsigned long long* counters, void* stream);
/* pi3_cloud_pair_equations (csrc/cloud_icp.hip): the normal equations of one ICP step from the pairs of a search.
 * queries f32 [m][3]: the estimate, already moved by the current transform (the rows pi3_cloud_nearest was given);
 * points f32 [n][3]: the indexed cloud in its original order; idx int32 [m], d2 f64 [m] as pi3_cloud_nearest wrote them.
 * centre HOST f64 [3] (finite); Rn HOST f64 [9] row-major or NULL (= identity), read in mode 2 only; both are read
 * during the call.  normals_of: 0 point to point (normals ignored); 1 normals f32 [n][3] read at idx[i] (the target's);
 * 2 normals f32 [m][3] read at i (the source's), each first rotated by Rn.
 * Pair i takes part when 0 <= idx[i] < n (else "unmatched"), d2[i] <= trim_dist trim_dist (inclusive, the product formed
 * once in f64; else "trimmed") and, in modes 1 and 2, the (rotated) normal a has 0 < (a0 a0 + a1 a1) + a2 a2 < inf (else
 * "normal rejected": zero, NaN, inf); n = a / sqrt(that), in f64.  With p = query, q = points[idx], x = p - centre,
 * e = p - q (f64), the motion p' = p + w x x + l x + t about centre and J = [ -[x]x | x | I ] (parameters w (3), l, t (3)):
 *   mode 0:     A += J^T J,  b += J^T e,  r2 += e.e;
 *   modes 1, 2: j = J^T n = (x x n, x.n, n),  r = n.e:   A += j j^T,  b += j r,  r2 += r r.
 * out DEVICE f64 [40] = the 28 entries of A's upper triangle row-major, the 7 of b, r2, the sum of e.e (in every mode),
 * 3 zeros.  counters DEVICE uint64 [4] = pairs used, unmatched, trimmed, normal rejected; zeroed by the call.
 * The sums are bitwise reproducible (no floating-point atomics): a workgroup covers 4096 consecutive queries and writes
 * one row of 40 doubles into partials (DEVICE f64 [partial_rows][40], partial_rows >= ceil(m / 4096):
 * ops.cloud_icp_partial_rows; fewer: PI3_ERR_WORKSPACE), a second launch of one workgroup adds the rows in a fixed
 * order.  m == 0 launches nothing and writes zeros.  Bad arguments (a negative size, normals_of outside 0..2, NULL
 * where a row array is needed, trim_dist not finite or < 0, a centre or Rn that is not finite) launch nothing and leave
 * out and counters untouched.  No allocation, no synchronisation. */
int pi3_cloud_pair_equations(const float* queries, long m, const float* points, long n, const int* idx,
                             const double* d2, double trim_dist, const double* centre, const float* normals,
                             int normals_of, const double* Rn, double* partials, long partial_rows, double* out,
                             unsigned long long* counters, void* stream);

/* ---- nearest triangle of a mesh (csrc/mesh_nn.hip): the exact radius-bounded point-to-surface distance, through the
 * cell grid of pi3_cloud_index_build (same table form, quantiser and inv_cell).  vertices f32 [V][3], faces int32 [F][3].
 * A triangle gets a row (its face index, int32) in every cell of its axis-aligned bounding box; it is dropped (counted,
 * no row, never returned) when a vertex index is outside [0, V), a vertex is not finite or outside the quantiser's
 * |k| < 2^20, or the f64 squared norm of ab x ac is 0.  The number of rows is not known in advance: two calls.
 * pi3_mesh_index_count: clears the table (capacity slots of 64 B, a power of two, more than the cells the mesh covers),
 * writes packed f32 [F][12] = a, b, c, 2 spare, the face index as int32 (-1 = dropped), and counts the rows per cell
 * unless their total exceeds max_rows (1 .. 2^31 - 1; then the table stays clear).  counters: DEVICE uint64 [8], zeroed
 * by the call = dropped triangles, cells, (triangle, cell) pairs that found no free slot, largest cell (written by the
 * fill), total rows (a box of 2^32 cells or more counts as 2^32), 3 spare.  F == 0 leaves an empty table.
 * pi3_mesh_index_fill: table, packed, F, inv_cell as the count call left them, rows int32 [n_rows] with n_rows the
 * count call's total; gives every occupied cell its rows and writes them; writes the largest cell into `counters` (the
 * count call's array, not zeroed).  The order of the rows is not defined.
 * pi3_mesh_nearest: queries f32 [m][3] -> d2 f64 [m], face int32 [m], closest f32 [m][3]: over the triangles in the 27
 * cells around the query, the closest point by Ericson's region tests (Real-Time Collision Detection 5.1.5) in f64
 * without contraction, the exact operation order stated at the top of mesh_nn.hip; candidate when d2 <= max_dist^2
 * (inclusive; a d2 that is not finite never is); the smallest d2 wins, among equal d2 the smallest face index.  Without
 * a candidate, or for a dropped query: +inf, -1, (0, 0, 0).  NaN is written nowhere.  max_dist * inv_cell <= 0.9 as
 * for pi3_cloud_nearest.  counters: DEVICE uint64 [4] = dropped queries, matched, beyond, triangle evaluations; zeroed
 * by the call.  m == 0 launches nothing; F == 0: every query is beyond.  Bad arguments launch nothing.  No
 * allocation, no synchronisation. */
int pi3_mesh_index_count(const float* vertices, long V, const int* faces, long F, float inv_cell, void* table,
                         long capacity, float* packed, long max_rows, unsigned long long* counters, void* stream);
int pi3_mesh_index_fill(void* table, long capacity, const float* packed, long F, float inv_cell, int* rows, long n_rows,
                        unsigned long long* counters, void* stream);
int pi3_mesh_nearest(const void* table, long capacity, const int* rows, long n_rows, const float* packed, long F,
                     float inv_cell, const float* queries, long m, double max_dist, double* d2, int* face,
                     float* closest, unsigned long long* counters, void* stream);
/* ---- area-weighted samples of a mesh's surface (csrc/mesh_sample.hip), a function of the mesh, the spacing and the
 * seed, bit for bit (the hash and the operation order are stated at the top of the file).
 * pi3_mesh_sample_counts: counts int64 [F] = floor(area / spacing^2 + u_f) with u_f in [0, 1) from (seed, face), at
 * most 2^31 - 1; 0 for a dropped face (index outside [0, V), a coordinate not finite, zero area).  counters: DEVICE
 * uint64 [4], zeroed by the call = dropped faces, 3 spare.
 * pi3_mesh_sample_points: offsets int64 [F + 1] = the exclusive prefix sums of counts (offsets[F] = n); sample
 * offsets[f] + j is sample j of face f: points f32 [n][3] uniform on the triangle, face int32 [n], normals f32 [n][3] =
 * the unit face normal by the winding.  F >= 1.  n == 0 launches nothing. */
int pi3_mesh_sample_counts(const float* vertices, long V, const int* faces, long F, double spacing,
                           unsigned long long seed, long long* counts, unsigned long long* counters, void* stream);
int pi3_mesh_sample_points(const float* vertices, long V, const int* faces, long F, const long long* offsets, long n,
                           unsigned long long seed, float* points, int* face, float* normals, void* stream);

/* ---- dense map -> camera views (csrc/render.hip): a z-buffered splat renderer for the voxel map.
 * points f32 [V][3] (the voxel centroids, in ascending key order), weights int32 [V] (or NULL: every voxel counts),
 * cams f64 [M][20] = world->camera 3x4 row-major (12), fx, fy, cx, cy, ortho flag (0 / 1), 3 spare.  zbuf uint64
 * [M][H][W]: filled with all ones (= empty) first; then every voxel does, per camera (f64, no contraction):
 *   skip when a coordinate is not finite or weights[i] < min_weight;
 *   xc = ((r00 x + r01 y) + r02 z) + t0, likewise yc, zc;  skip unless near < zc <= far;
 *   perspective:  u = fx (xc / zc) + cx, v = fy (yc / zc) + cy, r = splat_scale voxel_size fx / zc;
 *   orthographic: u = fx xc + cx,        v = fy yc + cy,        r = splat_scale voxel_size fx;
 *   r = min(max(r, 0.5), 16) (a clamp at 16 adds one to stats[1]);
 *   x0 = max(ceil(u - r), 0), x1 = min(floor(u + r), W - 1), same for y: pixel i has its centre at i; an empty range
 *   adds one to stats[0];
 *   every pixel of the footprint: zbuf = min(zbuf, float_bits((float)zc) << 32 | i)   (64-bit atomic).
 * The image does not depend on the order in which the atomics land.  V < 2^31, M <= 65535.  stats: DEVICE uint64 [4],
 * accumulated (the caller zeroes them): voxels without a pixel, radius clamps, non-empty pixels (resolve), spare. */
int pi3_render_splat(const float* points, const int* weights, long V, const double* cams, int M, int H, int W,
                     double voxel_size, double splat_scale, int min_weight, double near, double far,
                     unsigned long long* zbuf, unsigned long long* stats, void* stream);
/* zbuf [M][H][W] + colors uint8 [V][3] -> depth f32 [M][H][W] (0 where empty), color uint8 [M][H][W][3] (0 where
 * empty), index int32 [M][H][W] (the voxel's row, -1 where empty); stats[2] += the number of non-empty pixels. */
int pi3_render_resolve(const unsigned long long* zbuf, const unsigned char* colors, long V, int M, int H, int W,
                       float* depth, unsigned char* color, int* index, unsigned long long* stats, void* stream);

/* ---- surface normals of the dense voxel map (csrc/voxel_normals.hip).  The table's slot is full, so the normals live
 * beside it: nacc, caller-owned DEVICE memory of int64 [capacity][4] = Nx, Ny, Nz, cnt per slot, parallel to the table
 * and zeroed by the caller.  Every update is a 64-bit integer atomic add: the sums do not depend on the order in which
 * the atomics land.  Slots are looked up read-only; nothing here claims one, so the matching fusion call ran first on
 * the same inputs.  Arithmetic is f64 from the fp32 inputs, no contraction, every operation rounded on its own.
 * stats of the two fusion calls: DEVICE uint64 [4], accumulated (the caller zeroes them) = contributions, candidates
 * that could not contribute, degenerate normals, contributions whose slot was not found (0 after the matching fusion).
 *
 * pi3_voxel_fuse_pixel_normals: after pi3_voxel_fuse_pixels on the same points / conf / masks / N H W / threshold /
 * inv_voxel.  Pixel (f, y, x) is a candidate under that call's predicate (mask != 0, conf > conf_logit_thr, the three
 * axes quantise).  It contributes when 1 <= x <= W - 2, 1 <= y <= H - 2 and its neighbours (y, x +- 1), (y +- 1, x) of
 * the same frame are candidates too (else stats[1]):
 *   a = P(y, x + 1) - P(y, x - 1),  b = P(y + 1, x) - P(y - 1, x),  n = b x a  (nx = by az - bz ay, ...; with x right,
 *   y down, z forward it faces the camera);  l2 = (nx nx + ny ny) + nz nz;  no contribution unless l2 > 0 and finite
 *   (stats[2]);  l = sqrt(l2);  q_a = (int64) rint((n_a / l) * 32768), half to even;  nacc[slot] += (qx, qy, qz, 1). */
int pi3_voxel_fuse_pixel_normals(const void* table, long capacity, long long* nacc, const float* points,
                                 const float* conf, const unsigned char* masks, int N, int H, int W,
                                 float conf_logit_thr, float inv_voxel, unsigned long long* stats, void* stream);
/* After pi3_voxel_fuse_points on the same points (f32 [n][3], already in the world frame).  normals f32 [n][3] in the
 * cloud's own frame, nweights int32 [n], rot9 DEVICE f64 [9] row-major: the rotation of the cloud's similarity.  A row
 * with nweights > 0, a finite non-zero normal (else stats[2]) and a quantisable point (else stats[1]) adds
 *   nweights * q_a,  q_a = rint(((r_a0 nx + r_a1 ny) + r_a2 nz) * 32768) limited to +-2^31,  and nweights to cnt. */
int pi3_voxel_fuse_point_normals(const void* table, long capacity, long long* nacc, const float* points,
                                 const float* normals, const int* nweights, const double* rot9, long n, float inv_voxel,
                                 unsigned long long* stats, void* stream);
/* One row per occupied slot, or per occupied slot with keep_or_null[slot] != 0 (uint8 [capacity]): keys uint64 [V],
 * normals f32 [V][3] = (float)(N_a / sqrt((Nx Nx + Ny Ny) + Nz Nz)), (0, 0, 0) when cnt == 0 or the three sums are 0,
 * nweights int32 [V] = min(cnt, 2^31 - 1); at most max_out rows, in no defined order (sort by key on the host: that
 * lines the rows up with pi3_voxel_extract's).  stats: DEVICE uint64 [4], zeroed by the call = rows, rows that did not
 * fit max_out, stored rows with a non-zero normal, spare. */
int pi3_voxel_extract_normals(const void* table, long capacity, const long long* nacc, const unsigned char* keep_or_null,
                              unsigned long long* keys, float* normals, int* nweights, long max_out,
                              unsigned long long* stats, void* stream);
/* Element-wise over pi3_render_resolve's index int32 [M][H][W]; normals f32 [V][3] in the world frame, cams as
 * pi3_render_splat's.  A pixel with 0 <= idx < V and a finite non-zero normal:
 *   nc = R_wc n, nc_x = (c0 nx + c1 ny) + c2 nz, likewise nc_y (c4..c6) and nc_z (c8..c10);
 *   normal_rgb uint8 [M][H][W][3] = clamp(rint((nc + 1) * 127.5), 0, 255) per axis;
 *   shaded uint8 [M][H][W] = clamp(rint(255 * max(0, -nc_z)), 0, 255): a headlight along the optical axis.
 * Every other pixel is 0 in both.  stats: DEVICE uint64 [>= 1], accumulated; stats[0] += the shaded pixels. */
int pi3_render_shade(const int* index, const float* normals, long V, const double* cams, int M, int H, int W,
                     unsigned char* normal_rgb, unsigned char* shaded, unsigned long long* stats, void* stream);

/* ---- a triangle mesh of the fused voxel table (csrc/voxel_mesh.hip): an oriented-point signed field on the table's
 * lattice, meshed by surface nets; f64 / integer arithmetic that tests/dense_mesh_ref.py reproduces byte for byte.
 * table / capacity / nacc / keep_or_null as above.  A SOURCE voxel is an occupied (and kept) slot with W >= 1, cnt > 0
 * and a non-zero normal sum.  The cell table is caller-owned DEVICE memory: cells uint64 [cell_capacity] (a power of
 * two) and verts uint32 [cell_capacity][8].  stats: DEVICE uint64 [12]; every call zeroes the entries it writes.
 *
 * pi3_voxel_mesh_cells: clears `cells` and inserts the keys of the 27 cells around every source voxel.
 *   stats[0] = source voxels, [1] = cells, [2] = inserts that found no slot within min(cell_capacity, 256)
 *   probes (the table is too small: nothing was written for them; grow it and call again).  cells_or_null = NULL: stats[0] only.
 * pi3_voxel_mesh_vertices: one vertex per cell with a sign change on one of its 12 edges -> verts.
 *   stats[3] = vertices, [4] = quads, [5] = cell faces with four crossings (non-manifold edges).
 * pi3_voxel_mesh_extract: vertex rows vkeys uint64 [V] (the cell's key), vxyz f32 [V][3] (metres), vnrm f32 [V][3],
 *   vrgb uint8 [V][3], at most max_vertices; quad rows qkeys uint64 [Q] (the owner cell's key) and qcodes int32 [Q]
 *   = axis | flip << 2, at most max_quads; in no defined order.  The quad of owner i along axis a joins the cells
 *   i - e_b - e_c, i - e_c, i, i - e_b (b = (a + 1) % 3, c = (a + 2) % 3), counter-clockwise seen from +a, reversed
 *   under flip.  stats[6] = vertex rows, [7] = quad rows, [8] / [9] = rows of either kind that did not fit. */
int pi3_voxel_mesh_cells(const void* table, long capacity, const long long* nacc, const unsigned char* keep_or_null,
                         unsigned long long* cells_or_null, long cell_capacity, unsigned long long* stats, void* stream);
int pi3_voxel_mesh_vertices(const void* table, long capacity, const long long* nacc, const unsigned char* keep_or_null,
                            const unsigned long long* cells, long cell_capacity, double voxel_size, unsigned* verts,
                            unsigned long long* stats, void* stream);
int pi3_voxel_mesh_extract(const unsigned long long* cells, long cell_capacity, const unsigned* verts,
                           unsigned long long* vkeys, float* vxyz, float* vnrm, unsigned char* vrgb, long max_vertices,
                           unsigned long long* qkeys, int* qcodes, long max_quads, unsigned long long* stats,
                           void* stream);

/* ---- loop closure: which chunks see the same surface (csrc/chunk_overlap.hip).  Exact integers.
 * points f32 [P][3]: the dense clouds of all C chunks, already in the world frame, one after the other; offsets DEVICE
 * int64 [C + 1]: chunk c owns the rows offsets[c] .. offsets[c + 1] - 1 (a row before offsets[0] or from offsets[C] on
 * belongs to no chunk and is dropped).  table: caller-owned DEVICE memory of `capacity` 64-byte slots (a power of two,
 * >= 2 P), cleared by the call: key | seven 64-bit words of chunk bits, so C <= 448 (more: PI3_ERR_ARG).
 * Pass 1: every point is quantised as the voxel map quantises it, at inv_cell (k = floor(p * inv_cell) per axis in fp32;
 * dropped when not finite or |k| >= 2^20), claims the slot of its cell and ORs its chunk's bit into the words (64-bit
 * integer atomics).  Pass 2: for every occupied cell and every unordered pair i <= j of its bits, counts[i][j] and
 * counts[j][i] += 1; the diagonal is counted once: counts[i][i] = the cells chunk i occupies.  counts DEVICE uint64
 * [C][C] and counters DEVICE uint64 [4] = dropped points, occupied cells, points that found no slot (0 under the
 * capacity rule), the largest number of chunks in one cell; both zeroed by the call.  The result does not depend on the
 * order of the atomics nor on how pass 2 aggregates (in LDS up to 64 chunks, in global memory above).
 * P == 0 or C == 0 clears counts and counters and launches no pass.  Bad arguments (a negative size, C > 448, inv_cell
 * not finite or <= 0, a capacity that is no power of two or below 2 P, NULL where an array is needed) launch nothing and
 * leave the outputs untouched.  No allocation, no synchronisation. */
int pi3_chunk_cooccupancy(const float* points, long P, const long* offsets, int C, float inv_cell, void* table,
                          long capacity, unsigned long long* counts, unsigned long long* counters, void* stream);

/* ---- loop closure: the Sim(3) pose graph over the chunks (csrc/pose_graph.hip), f64, every array on the DEVICE.
 * nodes f64 [C][16] in / out: W_c, the row-major 4x4 similarity chunk c -> world (its fourth row is written 0 0 0 1).
 * centres f64 [C][3]: g_c, the point a node's step turns and scales about (the world centroid of its cloud).
 * Edge e = (i, j) = edges int32 [E][2]:  Z f64 [E][16] the measured similarity chunk j -> chunk i, edge_centres f64
 * [E][3] a centre c_e in chunk i's frame, info f64 [E][28] the upper triangle, row-major, of the symmetric 7x7
 * information matrix O_e, in the parameter order w (3), l, t (3) of pi3_cloud_pair_equations.
 *   chart([sR | tau], c) = (rotation vector of R, ln s, tau - c + sR c);  r_e = chart(W_i^-1 W_j Z_e^-1, c_e);
 *   F = sum_e r_e^T O_e r_e.       An edge with an index outside [0, C) or with i == j is left out.
 * Levenberg-Marquardt with analytic Jacobians: node k steps by d_k in R^7 as W_k <- inc(d_k, g_k) W_k,
 * inc(x, g) = [ e^l exp([w]x) | g + t - e^l exp([w]x) g ].  fixed uint8 [C]: a node with fixed[c] != 0, and a free node
 * without an edge, keeps its value (identity rows in the system).  The dense 7C x 7C normal matrix is written one block
 * row per node with the edges in index order (no floating-point atomics: two runs give the same bits);
 * (H + lambda diag H) d = -g by Cholesky.  Per iteration: a factorisation that fails multiplies lambda by 10 (status 2
 * when lambda is 1e12 already); max |d| < 1e-9 converges and applies that last d; a candidate whose F differs from the
 * current one by no more than 1e-12 F converges and is applied; one with a smaller F is accepted (lambda / 10, at
 * least 1e-12); else lambda * 10 (at most 1e12).  lambda starts at 1e-4; decision and lambda live in the workspace, the call never waits for the device.
 * out f64 [16] = final F, initial F, iterations, accepted steps, final lambda, status (0 converged, 1 max_iterations
 * reached, 2 factorisation failed at the largest lambda: the nodes then hold their input values), 10 zeros.
 * max_iterations == 0 leaves the nodes as they are (status 1).  workspace: DEVICE f64 [workspace_doubles], at least
 * what pi3_pose_graph_workspace reports through *doubles (fewer: PI3_ERR_WORKSPACE); 49 C^2 of it is the matrix.
 * 1 <= C <= 448, E >= 0.  Bad arguments launch nothing and leave nodes and out untouched.  No allocation. */
int pi3_pose_graph_workspace(int C, int E, long* doubles);
int pi3_pose_graph_sim3(double* nodes, const double* centres, int C, const int* edges, const double* Z,
                        const double* edge_centres, const double* info, int E, const unsigned char* fixed,
                        int max_iterations, double* workspace, long workspace_doubles, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PI3SLAM_HIP_H */
