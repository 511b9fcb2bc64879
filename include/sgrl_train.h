/* sgrl_train.h -- C ABI of the dense products the TD3 update back-propagates through (gfx950).
 *
 * What it replaces: the `torch.nn.Linear` forward / backward calls inside the SET actor and critic when `Agent.update`
 * (reference src/agent.py:117-183) differentiates through them (reference src/SEActor.py:34-287, src/SECritic.py:8-124;
 * this repository's differentiable module is sgrl_amd/set_policy.py).  At the update's size -- batch 100 x 7..14 limbs = 700..1400
 * rows (x 3 for the vector channels) -- the vendor libraries spend most of the update inside a handful of single-workgroup
 * launches (a 256 x 256 macro tile looping over a 2 100-long contraction for a 30 x 128 weight gradient: 165 us); the kernels
 * behind this header are built for the latency of small products instead (32 x 32 output tiles, 128-deep k-tiles).
 *
 * Arithmetic: the float32 matrix instruction (exact float32 products, float32 accumulation); partial sums (the four waves of a
 * workgroup, the splits of a long weight-gradient contraction) are added in a fixed order: results are bit-reproducible.
 *
 * All pointers are DEVICE pointers owned by the caller; rows are `ld*` floats apart; no alignment is required (16-byte aligned
 * rows take the vector path).  `ws` (backward only; may be null: no split then) is scratch for split weight-gradient contractions:
 * sgrl_train_ws_floats() floats, ZERO filled before the first call; every call leaves its counter region zero again, so one
 * buffer serves any number of consecutive calls ON ONE STREAM.  Calls on different streams need different buffers.
 * Error codes as in sgrl.h; message via sgrl_train_last_error().  No CPU fallback.
 */
#ifndef SGRL_TRAIN_H
#define SGRL_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t sgrl_train_ws_floats(void);

/* y[M, N] = act(x[M, K] . w[N, K]^T + bias[N]) / rowdiv[M]; bias and rowdiv may be null; relu != 0 applies max(., 0)
 * (torch.nn.functional.linear, the ReLU that follows it, and the `/ F_norm` of reference SEActor.py:101,117 in one launch) */
int sgrl_linear_forward(const float* x, int ldx, const float* w, int ldw, const float* bias, const float* rowdiv, float* y,
                        int ldy, int M, int N, int K, int relu, void* stream);

/* sgrl_linear_forward with two optional fusions of what follows the product in the SET layers (one launch instead of two):
 *   addend [M, N] (row stride ldadd): y += addend after the epilogue -- the residual of the vector stream, g + linear5(.)
 *     (reference SEActor.py:110);
 *   tail [M, ntail]: y[m][N + j] = tail[m][j] -- columns appended to the product's N (y has N + ntail <= ldy columns): the
 *     gravity / direction pair behind the 30 projected channels, z = [proj(x) | gdir] (reference SEActor.py:93-94), or the scalar
 *     stream behind the invariant features, c = [inv | ng] (SEActor.py:98, 101); any ntail > 0.
 * The twin form does the same for the two critics' layers in one launch. */
int sgrl_linear_forward_fused(const float* x, int ldx, const float* w, int ldw, const float* bias, const float* rowdiv,
                              const float* addend, int ldadd, const float* tail, int ntail, float* y, int ldy, int M, int N, int K,
                              int relu, void* stream);
int sgrl_linear_forward_twin_fused(const float* x0, const float* x1, int ldx, const float* w0, const float* w1, int ldw, const float* b0,
                                   const float* b1, const float* rd0, const float* rd1, const float* add0, const float* add1, int ldadd,
                                   const float* tail0, const float* tail1, int ntail, float* y0, float* y1, int ldy, int M, int N, int K,
                                   int relu, void* stream);

/* Backward of the call above (`y` = its output, needed when relu != 0 or drowdiv != null; relu and rowdiv exclude each other).
 * g = dy masked by (y > 0) if relu, divided row-wise by rowdiv if given.
 *   dx[M, K]    = g . w                                  (skipped when dx == null)
 *   dw[N, K]    = g^T . x                                (skipped when dw == null)
 *   db[N]       = column sums of g                       (skipped when db == null)
 *   drowdiv[M]  = -(sum_n dy[m][n] y[m][n]) / rowdiv[m]  (skipped when drowdiv == null) */
int sgrl_linear_backward(const float* dy, int lddy, const float* y, int ldyo, int relu, const float* rowdiv, const float* x,
                         int ldx, const float* w, int ldw, float* dx, int lddx, float* dw, int lddw, float* db,
                         float* drowdiv, int M, int N, int K, float* ws, void* stream);
/* The same with the ReLU of the layer BELOW folded into the input gradient's epilogue: x_relu != 0 says that this layer's input x is
 * the output of a ReLU layer (x = max(., 0): linear1 -> ReLU -> linear2 of the reference's feed-forward pairs, SEActor.py:101-121),
 * and dx comes out masked by x > 0 -- which is the gradient that layer's backward needs, so it is then called with relu = 0 and
 * reads no mask in its two products (mask applied once per element here instead of once per k-tile there, twice).  The twin form
 * takes the two inputs x0 / x1 (both null: no mask). */
int sgrl_linear_backward_xrelu(const float* dy, int lddy, const float* y, int ldyo, int relu, const float* rowdiv, const float* x,
                               int ldx, const float* w, int ldw, float* dx, int lddx, float* dw, int lddw, float* db,
                               float* drowdiv, int M, int N, int K, int x_relu, float* ws, void* stream);

/* The same with the input gradient ACCUMULATED: acc_dx != 0 adds g . w (masked as above) onto what dx already holds instead of
 * overwriting it -- a tensor that feeds several linear layers (the vector stream g into g_proj and vg_proj, the invariant features c
 * into linear3 and linear1: reference SEActor.py:93-121) collects their input gradients in one buffer, product by product, without
 * the element-wise additions autograd would launch (sgrl_amd/train_ops.py fan_out).  Same stream: the products run in order. */
int sgrl_linear_backward_acc(const float* dy, int lddy, const float* y, int ldyo, int relu, const float* rowdiv, const float* x,
                             int ldx, const float* w, int ldw, float* dx, int lddx, float* dw, int lddw, float* db,
                             float* drowdiv, int M, int N, int K, int x_relu, int acc_dx, float* ws, void* stream);

/* The weight (+ bias) gradients of several layers in one launch per 12 layers: dw = g^T x, db = column sums of g, g as in
 * sgrl_linear_backward (which then is called with dw = db = null).  They are not on the backward pass's critical path -- only the
 * optimizer needs them -- so a caller may collect the descriptors during the pass and issue them together at its end. */
typedef struct sgrl_wgrad_desc {
  const float* dy; const float* y; const float* rowdiv; const float* x;   /* y: the forward's output, read when relu != 0 */
  float* dw; float* db;                                                    /* db may be null */
  int32_t lddy, ldy, ldx, lddw, M, N, K, relu;
} sgrl_wgrad_desc;
int sgrl_linear_wgrad_group(int n, const sgrl_wgrad_desc* d, float* ws, void* stream);

/* Twin products: the same layer of the reference's two critics (SECritic.py:8-124: critic1 / critic2, two TransformerModels on one
 * batch; agent.py:150-160 updates both from one loss) in ONE launch -- two argument sets of identical shape, the workgroup's z index
 * picks one.  Forward: y_i = act(x_i w_i^T + b_i) / rd_i; input gradient (and the row divisor's): dx_i = g_i w_i with g_i = dy_i
 * masked by y_i > 0 (relu) or divided by rd_i, drd_i[m] = -(dy_i[m] . y_i[m]) / rd_i[m].  The weight gradients of both go
 * through sgrl_linear_wgrad_group.  b / rd / drd: both null or both given. */
int sgrl_linear_forward_twin(const float* x0, const float* x1, int ldx, const float* w0, const float* w1, int ldw, const float* b0,
                             const float* b1, const float* rd0, const float* rd1, float* y0, float* y1, int ldy, int M, int N, int K,
                             int relu, void* stream);
int sgrl_linear_dgrad_twin(const float* dy0, const float* dy1, int lddy, const float* y0, const float* y1, int ldyo, int relu,
                           const float* rd0, const float* rd1, const float* w0, const float* w1, int ldw, float* dx0, float* dx1,
                           int lddx, float* drd0, float* drd1, int M, int N, int K, void* stream);
int sgrl_linear_dgrad_twin_xrelu(const float* dy0, const float* dy1, int lddy, const float* y0, const float* y1, int ldyo, int relu,
                                 const float* rd0, const float* rd1, const float* w0, const float* w1, int ldw, float* dx0, float* dx1,
                                 int lddx, float* drd0, float* drd1, const float* x0, const float* x1, int ldx, int M, int N, int K,
                                 void* stream);
int sgrl_linear_dgrad_twin_acc(const float* dy0, const float* dy1, int lddy, const float* y0, const float* y1, int ldyo, int relu,
                               const float* rd0, const float* rd1, const float* w0, const float* w1, int ldw, float* dx0, float* dx1,
                               int lddx, float* drd0, float* drd1, const float* x0, const float* x1, int ldx, int M, int N, int K,
                               int acc_dx, void* stream);

/* Gram invariants of M nodes' three 32-vectors z[M, 3, 32] (reference SEActor.py:94-98): gram[M, 1024] = vec(Z'Z),
 * fn[M] = ||Z'Z||_F + 1; and their backward: dz = Z (D + D'), D = dgram + (dfn / ||Z'Z||_F) Z'Z (dgram or dfn may be null). */
int sgrl_gram_forward(const float* z, float* gram, float* fn, int M, void* stream);
int sgrl_gram_backward(const float* z, const float* dgram, const float* dfn, const float* fn, float* dz, int M, void* stream);
/* The same invariants on the lower triangle of the symmetric Z'Z only: tri[M, 528], tri[m][a (a + 1) / 2 + b] = (Z'Z)[a][b], a >= b
 * (fn as above, the norm of the FULL matrix).  A linear layer W on vec(Z'Z) equals W' on tri(Z'Z) with the mirror columns of W added
 * (sgrl_sym_fold), so its three products run over 528 columns instead of 1 024; dz = Z S with S[a][b] = S[b][a] = dtri[k] +
 * 2 (dfn / ||Z'Z||_F) (Z'Z)[a][b], the diagonal with 2 dtri[k].
 * sgrl_sym_fold: n <= 16 matrices per launch.  unfold == 0: wtri[i][rows[i], 528] = fold of w[i][rows[i], 1024] (W'[r][k] = W[r][a 32 + b] +
 * W[r][b 32 + a], the diagonal once); unfold != 0: w[i][r][a 32 + b] = w[i][r][b 32 + a] = wtri[i][r][k] -- the gradient of the fold
 * (w is then written, wtri read). */
int sgrl_gram_tri_forward(const float* z, float* tri, float* fn, int M, void* stream);
int sgrl_gram_tri_backward(const float* z, const float* dtri, const float* dfn, const float* fn, float* dz, int M, void* stream);
int sgrl_sym_fold(int n, const float* const* w, float* const* wtri, const int* rows, int unfold, void* stream);

/* Equivariant contraction of M nodes' three 32-vectors with their 32 x 32 matrices (reference SEActor.py:108-110, 262-264):
 * t[M, 3, 32] = z[M, 3, 32] . mat[M, 32, 32] per node; backward: dz = dt . mat', dmat = z' . dt. */
int sgrl_zmat_forward(const float* z, const float* mat, float* t, int M, void* stream);
int sgrl_zmat_backward(const float* z, const float* mat, const float* dt, float* dz, float* dmat, int M, void* stream);

/* Residual + LayerNorm over 128 columns (reference SEActor.py:90-91, 113-114: norm1(ng + attention update), norm2(ng + feed-forward
 * update); SEActor.py:164: the encoder's final norm, res = null):  y = LayerNorm(x + res) * w + b, eps inside the square root.
 * `nets` (1 or 2) networks stacked along the row axis, `rows` rows each ([nets * rows, 128]); network i uses w_i, b_i [128].
 * xhat [nets * rows, 128] (the normalised rows) and rstd [nets * rows] are what the backward needs (both null: not saved).
 * Backward: dx [nets * rows, 128] = the gradient of x AND of res; dw_i = sum_rows dy xhat, db_i = sum_rows dy (written, not
 * accumulated; null = not wanted; rows summed in a fixed order: bit-reproducible).  One launch each. */
int sgrl_add_ln_forward(const float* x, const float* res, const float* w0, const float* b0, const float* w1, const float* b1, float* y,
                        float* xhat, float* rstd, int rows, int nets, float eps, void* stream);
int sgrl_add_ln_backward(const float* dy, const float* xhat, const float* rstd, const float* w0, const float* w1, float* dx, float* dw0,
                         float* db0, float* dw1, float* db1, int rows, int nets, void* stream);

/* Three traversal-index embeddings concatenated (reference SEActor.py:18-31, ConcatPositionalEmbedding): idx [3, L] int64 (one index
 * vector per table, all < rows), w_t [rows, n_t], n0 + n1 + n2 <= 128:  out[l][:] = w0[idx[0][l]] | w1[idx[1][l]] | w2[idx[2][l]].
 * Backward: dw_t [rows, n_t] written densely (rows no limb points at receive zero; null = not wanted), limbs summed in order. */
int sgrl_embed3_forward(const long long* idx, const float* w0, const float* w1, const float* w2, int n0, int n1, int n2, float* out, int L,
                        void* stream);
int sgrl_embed3_backward(const long long* idx, const float* dout, float* dw0, float* dw1, float* dw2, int n0, int n1, int n2, int L, int rows,
                         void* stream);

/* Optimizer steps over a device TABLE of tensors instead of torch's multi-tensor launches (reference agent.py:161-177:
 * clip_grad_norm_ + Adam.step; common/functional.py:7-10: soft target update).  table: n_tensors rows of six 64-bit words
 * (param*, grad*, exp_avg*, exp_avg_sq*, step* (one float, the tensor's step count), numel); chunks: n_chunks pairs of int32
 * (row, first element), each covering at most sgrl_optim_chunk() elements of one tensor.
 *   sgrl_optim_clip_adam: max_norm > 0: total = sqrt(sum of grad^2 over every row), grads *= min(1, max_norm / (total + 1e-6)) in
 *     place (torch.nn.utils.clip_grad_norm_); every step += 1; Adam exactly as torch's fused kernel (no weight decay, no amsgrad):
 *     m = lerp(m, g, 1 - b1), v = b2 v + (1 - b2) g^2, p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
 *     scratch: 1 + n_chunks floats (total of squares, partials).  Three launches (two without clipping), fixed summation order.
 *     Non-finite gradients go the way clip_grad_norm_ sends them (its torch.clamp(coef, max=1.0) lets a NaN through): a NaN
 *     anywhere gives a NaN total and a NaN factor, so every gradient, moment and parameter of the table becomes NaN; an infinite
 *     total gives the factor 0 (the infinite element itself becomes NaN, every other gradient 0).  Finite totals: min(1, .) exactly.
 *   sgrl_optim_lerp: rows (dst*, src*, -, -, -, numel): dst = dst (1 - tau) + tau src.  One launch. */
int sgrl_optim_chunk(void);
int sgrl_optim_clip_adam(const void* table, int n_tensors, const void* chunks, int n_chunks, double lr, double beta1, double beta2, double eps,
                         float max_norm, float* scratch, void* stream);
int sgrl_optim_lerp(const void* table, const void* chunks, int n_chunks, float tau, void* stream);

/* Limb attention of B environments with L <= 14 limbs, 2 heads x 128 channels (reference subequivariant_attentions.py:90-151
 * between the projections).  qkv [B, L, 768] = q | k | v as the stacked projection leaves them (q is multiplied by `scale` inside);
 * the vector values are given in parts and never concatenated: vgp [B, L, 3, 252] (126 projected channels per head) and gdir
 * [B, L, 3, 2] (channels 126, 127 of both heads); bias [2, L, L] or null.
 *   w[b][h][i][:] = softmax_j(scale q_i . k_j + bias),  o[b][i][c] = sum_j w[h(c)] v[j][c],  og[b][i][s][c] = sum_j w[h(c)] vg[j][s][c]
 * w [B, 2, L, L] is returned for the backward, which yields dqkv [B, L, 768], dvgp [B, L, 3, 252], dgdh [B, L, 3, 2 heads, 2] (the
 * gradient of gdir per head: sum over the heads) and ds [B, 2, L, L] (the score gradient: its sum over the environments is the
 * gradient of `bias`). */
int sgrl_attention_forward(const float* qkv, const float* vgp, const float* gdir, const float* bias, float scale, float* w,
                           float* o, float* og, int B, int L, void* stream);
int sgrl_attention_backward(const float* qkv, const float* vgp, const float* gdir, float scale, const float* w, const float* d_o,
                            const float* d_og, float* dqkv, float* dvgp, float* dgdh, float* ds, int B, int L, void* stream);

/* Limb attention of the SWAT networks (swat_policy._SelfAttention between in_proj and out_proj): B environments with 1 <= L <= 15
 * limbs (SGRL_SWAT_MAX_LIMBS), 2 heads x 64 channels.  qkv [B, L, 384] = q | k | v as in_proj leaves them (q in columns 0..127, k
 * in 128..255, v in 256..383; head h owns columns 64 h .. 64 h + 63 of each; q is multiplied by `scale` inside); bias [2, L, L] or
 * null.
 *   w[b][h][i][:] = softmax_j(scale q_i . k_j + bias[h][i][j]),  o[b][i][64 h + d] = sum_j w[b][h][i][j] v[b][j][64 h + d]
 * w [B, 2, L, L] is returned for the backward, which takes d_o [B, L, 128] and yields dqkv [B, L, 384] and ds [B, 2, L, L] (the score
 * gradient: its sum over the environments is the gradient of `bias`):
 *   dw = d_o v',  ds = w (dw - sum_j w dw),  dq = scale ds k,  dk = ds' (scale q),  dv = w' d_o.
 * One launch per call, no atomics, fixed summation order (bit-reproducible).  B <= 0, L outside 1..15 or a null pointer (other
 * than bias) returns SGRL_ERR_ARG before anything is launched. */
int sgrl_swat_attention_forward(const float* qkv, const float* bias, float scale, float* w, float* o, int B, int L, void* stream);
int sgrl_swat_attention_backward(const float* qkv, float scale, const float* w, const float* d_o, float* dqkv, float* ds, int B, int L,
                                 void* stream);

/* ---- counter-RNG dropout (sgrl_amd/swat_policy.py with dropout_rate > 0; csrc/dropout.hip, csrc/dropout_rng.h) -------------------
 * The reference's --dropout_rate reaches the SWAT networks only (StructureActor.py:130-134, StructureCritic.py:46, 60), at five
 * kinds of site: the position embedding (StructureActor.py:29), the softmax weights (attentions.py:163), dropout1 behind out_proj,
 * `dropout` between the ReLU and linear2, dropout2 behind linear2 (StructureActor.py:56-62).  Here a mask is a FUNCTION of four
 * numbers instead of a draw from a generator, so no pass stores one and a backward regenerates its forward's:
 *   word = replay_word(seed, step, 0x100 + site, i)       Philox4x32-10 as in sgrl_replay.h (stream ids 0 and 1 are the replay's);
 *                                                          i = row-major linear index in the tensor the dropout is applied to
 *   thr  = (uint64) floor((double) p * 4294967296.0)      p a float in [0, 1]
 *   keep = (uint64) word >= thr
 *   y    = keep ? x * (1.0f / (1.0f - p)) : 0.0f          p == 1: y = 0;  p == 0: y = x, bit for bit
 * seed: a host argument (the agent's seed).  step_dev: a DEVICE uint64 the kernel reads -- the update number, which the host never
 * has to know (td3.Agent increments it on the update's stream).  site: a host int in 0 .. 2^24 - 1, the running number of the
 * dropout call inside one update; the backward of a call passes the forward's (step, site).
 *
 * sgrl_dropout_forward: y[0 .. n) = dropout(x[0 .. n)), element-wise and OUT OF PLACE (overlapping x and y are refused), n >= 1 with
 * 64-bit indices; one Philox block serves four consecutive elements; 16-byte accesses when x and y are both 16-byte aligned,
 * scalar ones otherwise and for the last n mod 4 elements.  sgrl_dropout_backward: dx = dropout(dy) with the same mask -- the same
 * kernel.  One launch per call, every element written once: bit-reproducible.  A null pointer, n <= 0, p outside [0, 1] (a NaN
 * included) or a site outside its range returns SGRL_ERR_ARG before anything is launched. */
int sgrl_dropout_forward(const float* x, float* y, int64_t n, float p, uint64_t seed, const uint64_t* step_dev, int site, void* stream);
int sgrl_dropout_backward(const float* dy, float* dx, int64_t n, float p, uint64_t seed, const uint64_t* step_dev, int site, void* stream);

/* sgrl_swat_attention_forward / _backward with the softmax weights dropped, wd = dropout(w) over the index of w [B, 2, L, L]:
 *   forward:   o = wd v;  the w returned is UNDROPPED (the softmax Jacobian needs it) and no mask is stored;
 *   backward:  dw = (d_o v') keep / (1 - p),  ds = w (dw - sum_j w dw),  dv = wd' d_o,  dq = scale ds k,  dk = ds' (scale q).
 * An o row whose weights were all dropped is exact zeros.  Limits, argument checks (plus those of p, step_dev and site above), one
 * launch per call, no atomics and the fixed summation order are those of the pair above, whose kernels and bits are unchanged:
 * both pairs are instantiations of one template. */
int sgrl_swat_attention_forward_dropout(const float* qkv, const float* bias, float scale, float* w, float* o, int B, int L, float p,
                                        uint64_t seed, const uint64_t* step_dev, int site, void* stream);
int sgrl_swat_attention_backward_dropout(const float* qkv, float scale, const float* w, const float* d_o, float* dqkv, float* ds, int B, int L,
                                         float p, uint64_t seed, const uint64_t* step_dev, int site, void* stream);

/* ---- SMP networks (sgrl_amd/smp_policy.py `train_kernels`; csrc/smp_train.hip) --------------------------------------------------
 * What lies between the linear layers of the message-passing networks' differentiable passes, one launch per call, float32, on
 * `stream`, no host synchronisation, no atomics, no scratch; every output element is written exactly once in a fixed order
 * (bit-reproducible).  Limits as in sgrl_smp.h: SGRL_SMP_MAX_LIMBS = 16 nodes per level, SGRL_SMP_MAX_CHILDREN = 8, messages 32 wide.
 * An argument error returns SGRL_ERR_ARG with the function's name in the message BEFORE anything is launched: a null required
 * pointer, B (R) <= 0, a node count outside 1..16, `S` (the child slots: max_children) outside 1..8, a width outside the ranges
 * below, a table entry outside its source.
 *
 * Message gather of the n limbs of one tree level, rows [n, B, .]:
 *   out[j][b] = act([ own'(j, b) | seg_0 | ... | seg_{S-1} ])                                   out [n, B, W0 + 32 S]
 *   own [n, B, W0], W0 = 0 (no own part, own may be null), 32 or 64; own' = own / max(||own||, 1e-12) if normalize != 0 (F.normalize;
 *     inv [n, B] then receives 1 / max(||own||, 1e-12) for the backward), own otherwise;
 *   seg_s = 32 columns of src [n_src, B, Wsrc] (Wsrc a multiple of 32, <= 256) at row block node[j * S + s], columns off[j * S + s] ..
 *     + 31 (a multiple of 32); node = -1: zeros; src == null: all segments zero (n_src, Wsrc and the table's values are not read);
 *   act = tanh if act_tanh != 0, the identity otherwise.
 * node / off are HOST arrays of n * S int32 (sgrl_amd/smp_policy._Tree decides them: children bottom-up, the parent's slot top-down):
 * they are checked here and travel in the kernel's arguments -- no call copies anything to the device.
 * Backward, from d_out [n, B, W0 + 32 S] (and `out` when act_tanh, `own` and `inv` when normalize):
 *   d_own [n, B, W0] through tanh' and the normalisation's Jacobian (null: not wanted; must be null when W0 = 0);
 *   d_src [n_src, B, Wsrc], ALL of it: the 32-column group a segment read receives that segment's gradient, a group nobody read
 *     zeros (null: not wanted).  Two table entries reading the same group are refused (SGRL_ERR_ARG): plain stores, one writer. */
int sgrl_smp_gather_forward(const float* own, int W0, int normalize, const float* src, int n_src, int Wsrc, const int32_t* node,
                            const int32_t* off, int S, int act_tanh, float* out, float* inv, int n, int B, void* stream);
int sgrl_smp_gather_backward(const float* d_out, const float* out, const float* own, const float* inv, int W0, int normalize, int n_src,
                             int Wsrc, const int32_t* node, const int32_t* off, int S, int act_tanh, float* d_own, float* d_src, int n,
                             int B, void* stream);

/* Tail of the bottom-up module (smp_policy._up_message behind fc2; reference ModularActor.py:35-47): a [R, 64] = fc2's output,
 * w3 [32, 64], b3 [32]:  t = tanh(a) [R, 64] (stored),  z = w3 t + b3,  u = z / max(||z||, 1e-12) [R, 32],  inv [R] = 1 / max(||z||, 1e-12).
 * Backward from du [R, 32]: dz [R, 32] (the gradient at fc3's output: du through the normalisation) and da [R, 64] = (dz w3)(1 - t^2).
 * fc3's weight / bias gradients are dz^T t and the column sums of dz: sgrl_linear_wgrad_group with dy = dz, x = t. */
int sgrl_smp_up_tail_forward(const float* a, const float* w3, const float* b3, float* t, float* u, float* inv, int R, void* stream);
int sgrl_smp_up_tail_backward(const float* du, const float* u, const float* inv, const float* t, const float* w3, float* dz, float* da, int R,
                              void* stream);

/* F.normalize over the rows of x [R, W], 1 <= W <= 256: y = x / max(||x||, 1e-12), inv [R] = 1 / max(||x||, 1e-12).  Backward:
 * dx = (dy - y (y . dy)) inv; a row shorter than 1e-12 was divided by 1e-12 and its gradient is dy / 1e-12, as torch's is. */
int sgrl_row_normalize_forward(const float* x, float* y, float* inv, int R, int W, void* stream);
int sgrl_row_normalize_backward(const float* dy, const float* y, const float* inv, float* dx, int R, int W, void* stream);

/* ---- the losses of a TD3 update (sgrl_amd/td3.py Agent `loss_kernels`; csrc/td3_loss.hip) ---------------------------------------
 * Replaces, with one launch per call, the loss expressions of reference src/agent.py:150-176 and the autograd nodes behind them:
 *   critic_loss = F.mse_loss(current_Q1, target_Q) + F.mse_loss(current_Q2, target_Q)     (two reductions, an addition; five
 *                                                                                           element-wise launches going back)
 *   actor_loss  = -self.critic.Q1(obs_batch, self.actor(obs_batch)).mean()                 (a reduction, a negation; three back)
 * over n contiguous float32 elements each, n >= 1 (64-bit indices):
 *   d_k[i] = (double) q_k[i] - (double) target[i],  loss = (float)((sum d_1^2 + sum d_2^2) / n),
 *   dq_k[i] = (float)((double) g[0] * 2 d_k[i] / n);       neg_mean: loss = (float)(-sum q / n),  dq[i] = (float)(-(double) g[0] / n).
 * The forward reductions run in ONE workgroup of 256 threads: each sums its elements i = t (mod 256) in ascending order in
 * float64, a fixed-shape tree in LDS adds the 256 partial sums: no atomics, no scratch, the same bits run to run.  The backward
 * kernels are element-wise and write dq[0 .. n) only.  loss and g are DEVICE scalars: the host reads neither, so every call can be
 * recorded into a hipGraph.  A null pointer, n <= 0, or q1 / q2 / dq1 / dq2 overlapping target return SGRL_ERR_ARG before anything
 * touches the device. */
int sgrl_td3_twin_mse_forward(const float* q1, const float* q2, const float* target, int64_t n, float* loss, void* stream);
int sgrl_td3_twin_mse_backward(const float* q1, const float* q2, const float* target, int64_t n, const float* g, float* dq1, float* dq2,
                               void* stream);
int sgrl_td3_neg_mean_forward(const float* q, int64_t n, float* loss, void* stream);
int sgrl_td3_neg_mean_backward(int64_t n, const float* g, float* dq, void* stream);
int sgrl_td3_loss_launches(void);   /* 1 per call */

const char* sgrl_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
