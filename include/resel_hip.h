/* resel_hip.h - C ABI of the MI355X (gfx950) kernels behind the `offpolicy_rnn` layer/operator interface.
 *
 * Drop-in boundary for the full-trajectory recurrent SAC/TD3 update of FanmingL/Recurrent-Offpolicy-RL.
 * The reference has no native code of its own: its GPU path binds Triton kernels and three un-vendored
 * CUDA extensions from Python.  Each entry point below names the reference interface it replaces
 * (path:line in the reference checkout).  The Python binding is recurrent-offpolicy-rl_amd/offpolicy_rnn/hip/_lib.py
 * (ctypes); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator); nothing is
 *     allocated, freed or synchronised inside; all work is enqueued on `stream` (a hipStream_t);
 *   - activations are TOKEN-MAJOR: logical [B, L, C] with channel stride 1, token index tok = b*L + t and an
 *     explicit token stride `ld_*` in ELEMENTS (so column slices of a wider row-major matrix are passed
 *     without copies); per-token flags are dense [B*L] fp32; base pointers and ld must be 16-byte aligned
 *     (ld % 4 == 0) where noted;
 *   - fp32 everywhere unless a name says bf16; no float atomics: results are bitwise reproducible;
 *   - return value: 0 = enqueued, <0 = RESEL_E* (nothing enqueued).  Scratch is caller-provided; its size
 *     comes from the matching *_workspace_bytes() function.
 */
#ifndef RESEL_HIP_H
#define RESEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RESEL_OK 0
#define RESEL_EINVAL (-1)   /* unsupported shape / null pointer / misalignment */
#define RESEL_ELAUNCH (-2)  /* hipLaunchKernel reported an error */

typedef void* resel_stream_t; /* hipStream_t */

/* Library / device identification (used by the binding to fail loudly when the wrong build is loaded). */
int resel_abi_version(void);            /* bumps when a signature changes */
const char* resel_build_info(void);     /* "gfx950 <date> ..." */

/* Diagnostics for bench.py (off by default; the only global state of the library).  While enabled, the sequence-layer
 * kernels are dispatched with a (start, stop) HIP event pair bound to each dispatch on its own stream;
 * resel_profile_collect() synchronises those events, returns their summed duration and count and clears them.
 * kernel_id: one of RESEL_PROF_* (attn_q_kernel is counted as ATTN_FWD or ATTN_DQ by its mode; the gru slots cover the
 * persistent kernels or, on the per-step path, every step launch). */
enum {
    RESEL_PROF_SSCAN_FWD = 0, RESEL_PROF_SSCAN_BWD = 1, RESEL_PROF_ATTN_FWD = 2, RESEL_PROF_ATTN_DQ = 3, RESEL_PROF_ATTN_DKV = 4,
    RESEL_PROF_LINREC_REAL_FWD = 5, RESEL_PROF_LINREC_REAL_BWD = 6, RESEL_PROF_LINREC_COMPLEX_FWD = 7, RESEL_PROF_LINREC_COMPLEX_BWD = 8,
    RESEL_PROF_GRU_FWD = 9, RESEL_PROF_GRU_BWD = 10, RESEL_PROF_CONV_FWD = 11, RESEL_PROF_CONV_BWD = 12, RESEL_PROF_GEMM = 13,
    RESEL_PROF_SSCAN_FWD_LOCAL = 14, RESEL_PROF_SSCAN_BWD_LOCAL = 15,   /* time-parallel form: the local passes (+ carry) of a call */
    RESEL_PROF_SSCAN_GATE_FWD = 16, RESEL_PROF_SSCAN_GATE_BWD = 17, RESEL_PROF_SSCAN_GROUP_REDUCE = 18,   /* state groups (N > 64) */
    RESEL_PROF_NSLOTS = 19
};
int resel_profile_enable(int on);
int resel_profile_collect(int kernel_id, double* total_us, int* launches);

/* ------------------------------------------------------------------------------------------------------
 * smamba selective scan.  Replaces `selective_scan_cuda.fwd / .bwd` (modified Mamba CUDA extension with the
 * extra `start` reset input) bound at offpolicy_rnn/models/smamba/mamba_ssm/ops/selective_scan_interface_new.py:47
 * and :72; arithmetic spec = `selective_scan_ref`, same file :96-166.
 *   delta' = softplus(delta + delta_bias)            (delta_softplus = 1; 0: delta' = delta + delta_bias;
 *                                                      2: `delta` already IS softplus(raw + bias) - the producing GEMM's epilogue applied
 *                                                      it (resel_gemm_f32x act 3) - the forward uses it as it stands and the backward
 *                                                      returns the gradient with respect to the RAW value: x (1 - exp(-delta)))
 *                                                      + 4 (ABI 7): `A` holds the parameter A_log; the kernels form A = -exp(A_log)
 *                                                      themselves (reference smamba/mamba.py:187) and the backward returns dA_log)
 *   h_t    = exp(delta'_t * A) * (1 - start_t) * h_{t-1} + delta'_t * Bm_t * u_t          h: [Di, N]
 *   out_t  = (<Cm_t, h_t> + D * u_t) * silu(z_t)     (gate skipped when z == NULL, skip term when D == NULL)
 * u, delta, z, out: [B*L, Di] (ld_u, ld_delta, ld_z, ld_out; 16-byte aligned); A: [Di, N] dense;
 * Bm, Cm: [B*L, N] (ld_b, ld_c); D, delta_bias: [Di]; start: [B*L] or NULL.
 * Supported by these two entries: Di % 4 == 0, N in {4, 8, 16, 32, 64} (any other N: RESEL_EINVAL).  Every d_state from 1 to 256 runs on
 *   them through the state plan of the Python layer (hip/ops.py `sscan_state_plan`): N <= 64 zero-padded to the next native size (zero
 *   B / C columns: exact), 64 < N <= 256 as up to RESEL_SSCAN_MAX_GROUPS column groups, each one call here with z == NULL and D == NULL,
 *   joined by the "state groups" entries below.
 * ckpt (optional, for the backward): state checkpoints every RESEL_SSCAN_CKPT steps,
 *   resel_selective_scan_ckpt_bytes(B, L, Di, N) bytes.  last_state (optional): [B, Di, N].
 * time_segments: 0 = the library decides (one workgroup scans a whole row when B * Di / 64 rows x tiles fill the chip; small
 *   batches are cut into time segments scanned in parallel: local pass, carry of the segment states, final pass), 1 = never
 *   split, k > 1 = k segments; workspace: resel_selective_scan_fwd_workspace_bytes(...) for the same arguments (NULL if 0).
 */
#define RESEL_SSCAN_CKPT 8
size_t resel_selective_scan_ckpt_bytes(int B, int L, int Di, int N);
size_t resel_selective_scan_fwd_workspace_bytes(int B, int L, int Di, int N, int time_segments);
int resel_selective_scan_fwd(const float* u, int64_t ld_u, const float* delta, int64_t ld_delta,
                             const float* z, int64_t ld_z, const float* A,
                             const float* Bm, int64_t ld_b, const float* Cm, int64_t ld_c,
                             const float* D, const float* delta_bias, const float* start,
                             float* out, int64_t ld_out, float* ckpt, float* last_state, void* workspace,
                             int B, int L, int Di, int N, int delta_softplus, int time_segments,
                             void* amax_out, unsigned amax_epoch, resel_stream_t stream);

/* Backward of the above.  dout: [B*L, Di] (ld_dout).  Outputs: du, ddelta, dz: [B*L, Di] (dz may be NULL iff
 * z is NULL); dBm, dCm: [B*L, N]; dA: [Di, N]; dD, ddelta_bias: [Di] (NULL iff the input was NULL).
 * All outputs are overwritten (not accumulated).  workspace: resel_selective_scan_bwd_workspace_bytes(). */
size_t resel_selective_scan_bwd_workspace_bytes(int B, int L, int Di, int N, int time_segments);
int resel_selective_scan_bwd(const float* u, int64_t ld_u, const float* delta, int64_t ld_delta,
                             const float* z, int64_t ld_z, const float* A,
                             const float* Bm, int64_t ld_b, const float* Cm, int64_t ld_c,
                             const float* D, const float* delta_bias, const float* start,
                             const float* dout, int64_t ld_dout, const float* ckpt,
                             float* du, int64_t ld_du, float* ddelta, int64_t ld_ddelta, float* dz, int64_t ld_dz,
                             float* dBm, int64_t ld_db, float* dCm, int64_t ld_dc,
                             float* dA, float* dD, float* ddelta_bias, void* workspace,
                             int B, int L, int Di, int N, int delta_softplus, int time_segments,
                             void* amax_dz, void* amax_ddelta, unsigned amax_epoch, resel_stream_t stream);

/* State groups (d_state > 64).  States are independent given (u, delta, B, C) and meet only in <C, h>: group g scans its own columns of
 * (A, B, C) with z == NULL, D == NULL into parts[g], and these entries do what the groups share.  parts, du_parts, ddelta_parts: G dense
 * [M, Di] slabs, stride_g floats apart (stride_g % 4 == 0, >= M * Di); M = B * L tokens; every other [M, Di] operand has its own token
 * stride (% 4, >= Di) and a 16-byte aligned base; G in 1 .. RESEL_SSCAN_MAX_GROUPS.  Groups are summed in index order and dD is a
 * two-stage column sum in a fixed order: bitwise reproducible, no atomics on floats.  One pass over HBM each.
 *   gate_fwd:      out = (sum_g parts[g] + D u) * silu(z)      (z, D optional as in the scan; amax_out gets max |out|)
 *   gate_bwd:      g = dout * silu(z) - the `dout` of every group's backward -, dz = dout * silu'(z) * (sum_g parts[g] + D u),
 *                  dD = sum over tokens of g u.  z == NULL: g, dz, parts must be NULL and the groups take dout itself; D == NULL: dD
 *                  must be NULL; both NULL is RESEL_EINVAL (nothing to form).  workspace: resel_sscan_gate_bwd_workspace_bytes(M, Di)
 *                  bytes when D is given.  amax_dz gets max |dz|.
 *   group_reduce:  du = sum_g du_parts[g] + D g (the skip term's share; g = the pre-gate gradient, needed with D only),
 *                  ddelta = sum_g ddelta_parts[g], ddelta_bias = sum_g dbias_parts[g] ([G, Di] dense; both NULL or neither).
 *                  amax_ddelta gets max |ddelta|.
 * RESEL_EINVAL before the device is touched: a NULL / misaligned required operand, Di % 4 != 0, M < 1, G outside its range, a stride
 * that is not a multiple of 4 or is shorter than its row, a magnitude handle that is not 8-byte aligned. */
#define RESEL_SSCAN_MAX_GROUPS 4
int resel_sscan_gate_fwd(const float* parts, int64_t stride_g, int G, const float* u, int64_t ld_u, const float* D,
                         const float* z, int64_t ld_z, float* out, int64_t ld_out, int64_t M, int Di,
                         void* amax_out, unsigned amax_epoch, resel_stream_t stream);
size_t resel_sscan_gate_bwd_workspace_bytes(int64_t M, int Di);
int resel_sscan_gate_bwd(const float* dout, int64_t ld_dout, const float* parts, int64_t stride_g, int G,
                         const float* u, int64_t ld_u, const float* D, const float* z, int64_t ld_z,
                         float* g, int64_t ld_g, float* dz, int64_t ld_dz, float* dD, void* workspace, int64_t M, int Di,
                         void* amax_dz, unsigned amax_epoch, resel_stream_t stream);
int resel_sscan_group_reduce(const float* du_parts, const float* ddelta_parts, int64_t stride_g, const float* dbias_parts, int G,
                             const float* g, int64_t ld_g, const float* D, float* du, int64_t ld_du,
                             float* ddelta, int64_t ld_ddelta, float* dbias, int64_t M, int Di,
                             void* amax_ddelta, unsigned amax_epoch, resel_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * smamba depthwise causal conv1d + bias + SiLU on the masked input.  Replaces `causal_conv1d_cuda.causal_conv1d_fwd/bwd`
 * (selective_scan_interface_new.py:199,273) and the nn.Conv1d(groups=d_inner) + SiLU branch taken for d_conv > 4
 * (offpolicy_rnn/models/smamba/mamba.py:75-83, 210-212).
 *   y[tok, d] = silu(bias[d] + sum_k w[d, k] * mask[tok'] * x[tok', d]),  tok' = tok - (K-1) + k within the row b
 * x, y: [B*L, Di] (ld_x, ld_y); w: [Di, K] dense; bias: [Di] or NULL; mask: [B*L] or NULL.  1 <= K <= 32.
 * Backward: dx [B*L, Di] (ld_dx), dw [Di, K], dbias [Di]; workspace resel_causal_conv1d_bwd_workspace_bytes().
 */
int resel_causal_conv1d_fwd(const float* x, int64_t ld_x, const float* w, const float* bias, const float* mask,
                            float* y, int64_t ld_y, int B, int L, int Di, int K, int silu, void* amax_y, unsigned amax_epoch,
                            resel_stream_t stream);
size_t resel_causal_conv1d_bwd_workspace_bytes(int B, int L, int Di, int K);
int resel_causal_conv1d_bwd(const float* x, int64_t ld_x, const float* w, const float* bias, const float* mask,
                            const float* dy, int64_t ld_dy, float* dx, int64_t ld_dx, float* dw, float* dbias,
                            void* workspace, int B, int L, int Di, int K, int silu, void* amax_dx, unsigned amax_epoch,
                            resel_stream_t stream);
/* The same with TWO gradients of the output, summed on load (dy2 may be NULL): the conv output of the Mamba mixer feeds the scan AND
 * x_proj, so its gradient is the scan's du plus the x_proj input gradient - taken as two tensors there is no accumulating GEMM epilogue
 * (150 us against 67 for the plain form at 66 752 x 512 x 80) and no add pass. */
int resel_causal_conv1d_bwd2(const float* x, int64_t ld_x, const float* w, const float* bias, const float* mask,
                             const float* dy, int64_t ld_dy, const float* dy2, int64_t ld_dy2, float* dx, int64_t ld_dx,
                             float* dw, float* dbias, void* workspace, int B, int L, int Di, int K, int silu,
                             void* amax_dx, unsigned amax_epoch, resel_stream_t stream);

/* Member edition for `econv1d[_<K>]-<E>` (reference offpolicy_rnn/models/conv1d/econv1d.py: one nn.Conv1d over E * Di grouped channels,
 * channel e * Di + d = member e): the same kernels over member-major rows.  y, dy, dx: [E, rows_per_member, L, Di], row e * rpm + b
 * belongs to member e; x the same or, with x_shared = 1, [rows_per_member, L, Di] read by every member; w [E, Di, K], bias [E, Di] or NULL;
 * mask [rows_per_member * L], shared by the members, or NULL.  No activation.  E * rows_per_member <= 65535; everything else as above.
 * Backward: dw [E, Di, K], dbias [E, Di] per member (fixed summation order).  dx_sum (x_shared only, may be NULL): dense
 * [rows_per_member, L, Di] = sum over the members of dx, member 0 first; it needs dense dx (ld_dx == Di) and rows_per_member * L * Di < 2^31.
 * amax_dx: max |dx| over the per-member gradients (no bound on dx_sum).  (Added without an ABI bump: no existing signature changed.) */
int resel_member_conv1d_fwd(const float* x, int64_t ld_x, int x_shared, const float* w, const float* bias, const float* mask,
                            float* y, int64_t ld_y, int E, int rows_per_member, int L, int Di, int K,
                            void* amax_y, unsigned amax_epoch, resel_stream_t stream);
size_t resel_member_conv1d_bwd_workspace_bytes(int E, int rows_per_member, int L, int Di, int K);
int resel_member_conv1d_bwd(const float* x, int64_t ld_x, int x_shared, const float* w, const float* bias, const float* mask,
                            const float* dy, int64_t ld_dy, float* dx, int64_t ld_dx, float* dx_sum, float* dw, float* dbias,
                            void* workspace, int E, int rows_per_member, int L, int Di, int K,
                            void* amax_dx, unsigned amax_epoch, resel_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Fused residual add + LayerNorm / RMSNorm.  Replaces the Triton kernels `_layer_norm_fwd_1pass_kernel` /
 * `_layer_norm_bwd_kernel` (offpolicy_rnn/models/smamba/mamba_ssm/ops/triton/layernorm.py:65,196; CPU spec
 * layernorm_cpu.py:6-35).  rows M, width C (C % 4 == 0, C <= 2048), all dense [M, C].
 *   res_out = x (+ residual) ; y = (res_out - mean) * rstd * w + b      (rms: y = res_out * rstd * w (+ b))
 * residual / res_out / bias may be NULL.  stats: [M, 2] (mean, rstd) saved for the backward.
 * Backward: dres_in (optional, [M, C]) is the gradient arriving at res_out from downstream; dx receives the
 * gradient w.r.t. x (== w.r.t. residual).  dw, db: [C]; workspace resel_add_layernorm_bwd_workspace_bytes().
 * act (ABI 8): 1 = y = elu(.) of the above (the plain ELU that follows a gilr / lru layer, reference rnn_base.py:456-469, applied where the
 * layer's closing add + LayerNorm stores its output); the backward then takes the bias `b` and forms elu' from the recomputed
 * pre-activation (no extra tensor saved).  0 = none.
 */
int resel_add_layernorm_fwd(const float* x, const float* residual, const float* w, const float* b,
                            float* y, float* res_out, float* stats, int M, int C, float eps, int rms, int act,
                            void* amax_y, unsigned amax_epoch, resel_stream_t stream);
size_t resel_add_layernorm_bwd_workspace_bytes(int M, int C);
int resel_add_layernorm_bwd(const float* dy, const float* dres_in, const float* res, const float* w, const float* b,
                            const float* stats, float* dx, float* dw, float* db, void* workspace,
                            int M, int C, int rms, int has_bias, int act, void* amax_dx, unsigned amax_epoch, resel_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * LayerNorm over a token's E segments of C floats: the `ln+<act>` (E = 1) and `eln-<E>+<act>` tails of the dense stacks
 * (reference offpolicy_rnn/models/rnn_base.py:250-258,461-467; `eln` normalises all E x C features of a token jointly, weight [E, C]).
 * Segment e of token m of an operand lies at  base + m * ld_m + e * ld_e  (floats; every operand brings its own pair), so the
 * token-major [M, E C] output of a shared-input ensemble layer (ld_e = C, ld_m = E C) and the member-major [E, M, C] tensors of the
 * deeper layers (ld_e = M C, ld_m = C) are read and written where they are.  ld_e is not used when E == 1, ld_m not when M == 1.
 *   y = act((x - mean) * rstd * w + b),  mean / rstd over the token's E C values;  w, b: dense [E, C], b may be NULL.
 * act: 0 none, 1 ELU (alpha 1); the backward re-forms elu' from the recomputed pre-activation.  stats: [M, 2] (mean, rstd).
 * amax_y: optional magnitude handle, gets the bound sqrt(E C) max|w| + max|b| (as resel_add_layernorm_fwd); amax_dx: max |dx|.
 * dw [E, C]; db [E, C] or NULL (needs b); workspace resel_member_layernorm_bwd_workspace_bytes() (0 for a refused shape).
 * RESEL_EINVAL: a NULL / misaligned (16 B) operand, C % 4 != 0, E * C > 2048, a stride that is not a positive multiple of 4 or
 * with E * ld_e >= 2^31, act outside {0, 1}.
 */
int resel_member_layernorm_fwd(const float* x, int64_t ldx_e, int64_t ldx_m, const float* w, const float* b,
                               float* y, int64_t ldy_e, int64_t ldy_m, float* stats, int M, int E, int C, float eps, int act,
                               void* amax_y, unsigned amax_epoch, resel_stream_t stream);
size_t resel_member_layernorm_bwd_workspace_bytes(int M, int E, int C);
int resel_member_layernorm_bwd(const float* dy, int64_t ldg_e, int64_t ldg_m, const float* x, int64_t ldx_e, int64_t ldx_m,
                               const float* w, const float* b, const float* stats, float* dx, int64_t ldd_e, int64_t ldd_m,
                               float* dw, float* db, void* workspace, int M, int E, int C, int act,
                               void* amax_dx, unsigned amax_epoch, resel_stream_t stream);
/* Residual form: y = act(LN(x + res)), the closing add + joint member LayerNorm of the ensemble feed-forward block of `elru-<E>`
 * (reference offpolicy_rnn/models/lru/elru.py:226-229) in one pass.  x, res and xsum (out: x + res, what the backward reads as its `x`)
 * share the stride pair (ldx_e, ldx_m); everything else as resel_member_layernorm_fwd, which this is bit for bit when the sum is formed
 * beforehand.  Backward: resel_member_layernorm_bwd on xsum - its dx is the gradient of x and of res.  (Added without an ABI bump: no existing signature changed.) */
int resel_member_add_layernorm_fwd(const float* x, const float* res, float* xsum, int64_t ldx_e, int64_t ldx_m,
                                   const float* w, const float* b, float* y, int64_t ldy_e, int64_t ldy_m, float* stats,
                                   int M, int E, int C, float eps, int act, void* amax_y, unsigned amax_epoch, resel_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Linear-recurrence scans (gilr, lru).  Replace the Triton kernels
 *   fwd_sequential_scan / bwd_sequential_scan          offpolicy_rnn/models/gilr/scan_triton/real_rnn_tie_input_gate.py:9,67
 *   fwd_sequential_scan_complex / bwd_...               offpolicy_rnn/models/lru/scan_triton/complex_rnn.py:44,91
 * (CPU specs real_rnn_tie_input_gate_cpu.py:4-14, complex_rnn_cpu.py:4-26) with a time-parallel chunked scan.
 * real:    v' = act ? tanh(v) : v ; f' = (act ? sigmoid(f) : f) * (1 - start) ; h_t = f'_t h_{t-1} + (1 - f'_t) v'_t
 * complex: h_t = lambda (1 - start_t) h_{t-1} + gamma * (vr_t + i vi_t)       (lambda, gamma per channel)
 * h, hr, hi, dh*: dense [B, L, C]; start: [B*L] or NULL; h0*: [B, C] or NULL (zeros).
 * v, f / vr, vi and their gradients may be column blocks of a wider token-major matrix (ABI 8): `ld_u` / `ld_du` = floats between the
 * rows of consecutive tokens (>= C; C for dense tensors).  The layers hand in the [M, E C] output of their shared-input EnsembleLinear
 * in place (reference gilr.py:60-62 / lru.py:112-120 slice an [E, B, T, C] tensor) and receive the gradients in the same layout.
 * Backward outputs are gradients w.r.t. the PRE-activation v, f (real) / vr, vi, lambda, gamma (complex;
 * dlam_re, dlam_im, dgamma: [C], reduced over B and L).  No gradient flows into h0 (reference: complex_rnn.py:242).
 * amax_h / amax_du (optional magnitude handles, see resel_amax): max |h| (complex: over hr and hi) / max over dv and df.
 */
int resel_linrec_real_fwd(const float* v, const float* f, int64_t ld_u, const float* start, const float* h0, float* h,
                          int B, int L, int C, int fuse_act, void* amax_h, unsigned amax_epoch, resel_stream_t stream);
int resel_linrec_real_bwd(const float* v, const float* f, int64_t ld_u, const float* start, const float* h0, const float* h,
                          const float* dh, float* dv, float* df, int64_t ld_du, int B, int L, int C, int fuse_act,
                          void* amax_du, unsigned amax_epoch, resel_stream_t stream);
int resel_linrec_complex_fwd(const float* vr, const float* vi, int64_t ld_u, const float* lam_re, const float* lam_im,
                             const float* gamma, const float* start, const float* h0r, const float* h0i,
                             float* hr, float* hi, int B, int L, int C, void* amax_h, unsigned amax_epoch, resel_stream_t stream);
size_t resel_linrec_complex_bwd_workspace_bytes(int B, int L, int C);
int resel_linrec_complex_bwd(const float* vr, const float* vi, int64_t ld_u, const float* lam_re, const float* lam_im,
                             const float* gamma, const float* start, const float* h0r, const float* h0i,
                             const float* hr, const float* hi, const float* dhr, const float* dhi,
                             float* dvr, float* dvi, int64_t ld_du, float* dlam_re, float* dlam_im, float* dgamma,
                             void* workspace, int B, int L, int C, resel_stream_t stream);
/* Member edition of the complex scan for `elru-<E>` (reference offpolicy_rnn/models/lru/elru.py:103-188 expands lambda / gamma to
 * [E * B, L, C] and scans E * B rows): the E * rows_per_member rows are member-major, rows e * rpm .. (e + 1) * rpm - 1 take row e of the
 * [E, C] tables lam_re / lam_im / gamma; start [rows_per_member * L] is shared by the members, h0r / h0i [E * rpm, C] are per row.
 * Backward: dlam_re, dlam_im, dgamma [E, C], reduced per member over its rows and L in a fixed order.  E * rows_per_member <= 65535.
 * E = 1 is resel_linrec_complex_fwd / _bwd bit for bit.  (Added without an ABI bump: no existing signature changed.) */
int resel_linrec_complex_members_fwd(const float* vr, const float* vi, int64_t ld_u, const float* lam_re, const float* lam_im,
                                     const float* gamma, const float* start, const float* h0r, const float* h0i,
                                     float* hr, float* hi, int E, int rows_per_member, int L, int C,
                                     void* amax_h, unsigned amax_epoch, resel_stream_t stream);
size_t resel_linrec_complex_members_bwd_workspace_bytes(int E, int rows_per_member, int L, int C);
int resel_linrec_complex_members_bwd(const float* vr, const float* vi, int64_t ld_u, const float* lam_re, const float* lam_im,
                                     const float* gamma, const float* start, const float* h0r, const float* h0i,
                                     const float* hr, const float* hi, const float* dhr, const float* dhi,
                                     float* dvr, float* dvi, int64_t ld_du, float* dlam_re, float* dlam_im, float* dgamma,
                                     void* workspace, int E, int rows_per_member, int L, int C, resel_stream_t stream);

/* lru's per-channel parameters in one launch each way (reference offpolicy_rnn/models/lru/lru.py:104-110: exp / cos / sin / mul on [C]
 * tensors).  params_log [3, C] = (nu_log | theta_log | gamma_log) -> out [3, C] = (lam_re | lam_im | gamma) with
 * lambda = exp(-exp(nu_log)) (cos, sin)(exp(theta_log)), gamma = exp(gamma_log); bwd: dout [3, C] -> dparams_log [3, C].  (ABI 8) */
int resel_lru_params_fwd(const float* params_log, float* out, int C, resel_stream_t stream);
int resel_lru_params_bwd(const float* params_log, const float* dout, float* dparams_log, int C, resel_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * GRU recurrence on a hoisted input projection.  Replaces cuDNN/MIOpen GRU reached through
 * torch.nn.GRU(batch_first=True) (offpolicy_rnn/models/rnn_base.py:59,247; called at :453-454).
 * gi = x W_ih^T + b_ih: [B, L, 3H] dense (r, z, n blocks); w_hh: [3H, H]; b_hh: [3H]; h0: [B, H] or NULL.
 *   r = sig(gi_r + W_hr h + b_hr) ; z = sig(gi_z + W_hz h + b_hz) ; n = tanh(gi_n + r * (W_hn h + b_hn))
 *   h' = (1 - z) n + z h ;  h_all: [B, L, H].  gates (optional, training): [B, L, 4H] saves r, z, n and
 *   (W_hn h + b_hn) for the backward.  Supported: H % 16 == 0 and H <= 256, or H in {288, 320, 336, 352, 384, 416, 448, 480, 512,
 *   640, 768, 896, 1024};
 *   every other width from 1 to 1024 runs zero-padded on the next of these (resel_gru_pad_* below; the padding is exact).
 * The recurrence is T-sequential; each step is one launch (grid = H/16 unit slices x ceil(B/16) row groups)
 * enqueued back-to-back from C.  workspace: resel_gru_workspace_bytes() (re-laid-out W_hh slices, carry).
 * Backward returns the pre-activation gradients of BOTH projections: dgi [B, L, 3H] (w.r.t. gi) and
 * dgh [B, L, 3H] (w.r.t. W_hh h + b_hh); the caller finishes dW_hh = dgh^T h_prev and db_hh = sum dgh with one
 * library GEMM (they are plain GEMM/reduction shapes over B*L rows).  No gradient is produced for h0.
 */
size_t resel_gru_workspace_bytes(int B, int L, int H);
int resel_gru_seq_fwd(const float* gi, const float* w_hh, const float* b_hh, const float* h0,
                      float* h_all, float* gates, void* workspace, int B, int L, int H, resel_stream_t stream);
int resel_gru_seq_bwd(const float* w_hh, const float* h0, const float* h_all, const float* gates,
                      const float* dh_all, float* dgi, float* dgh, void* workspace,
                      int B, int L, int H, resel_stream_t stream);

/* N independent GRU recurrences (1 <= n_net <= 4, same B, L, H; each with its own gi, W_hh, b_hh, h0 and outputs) in ONE launch
 * sequence on one stream: one layout launch, one memset, and either one persistent launch over all L steps (network = outermost
 * part of the workgroup index) or, when n_net x (H/16) x ceil(B/4) workgroups are not co-resident or RESEL_GRU_PERSISTENT=0, L
 * launches with the network in grid.z.  resel_gru_multi_form() tells which: 1 persistent, 0 per step.
 * gi, w_hh, b_hh, h0, h_all, gates are HOST arrays of n_net device pointers, read during the call and handed to the kernels by
 * value (no device-side table, no copy: the call is capturable).  h0 and gates may be NULL as arrays or per entry (zero initial
 * state / nothing saved for a backward).  The per-step arithmetic of a network is that of resel_gru_seq_fwd: its outputs are
 * bit-identical to a call for that network alone.  workspace: resel_gru_multi_workspace_bytes(); behind the n_net re-laid-out
 * W_hh copies (3 H H floats each) every network has ceil(B/4) * 8 H exchange granules (8 bytes) and a 64-byte block whose
 * first int is its error word (non-zero: a bounded spin ran out, that network's output is poisoned with NaN).
 * There is no backward twin: the backward recurrences of an update belong to different optimizer steps (resel_gru_seq_bwd). */
size_t resel_gru_multi_workspace_bytes(int n_net, int B, int L, int H);
int resel_gru_multi_fwd(int n_net, const float* const* gi, const float* const* w_hh, const float* const* b_hh,
                        const float* const* h0, float* const* h_all, float* const* gates, void* workspace,
                        int B, int L, int H, resel_stream_t stream);
int resel_gru_multi_form(int n_net, int B, int H);

/* Zero padding of a GRU of true width H onto a kernel width Hk the entries above accept (1 <= H < Hk).  Padding is PER GATE BLOCK:
 * row g * Hk + j of a padded tensor is row g * H + j of the true one (j < H) and zero otherwise; W_hh is padded in its columns too.
 * A padded unit stays exactly 0 through the forward and receives exactly 0 in the backward, so the true units compute what they
 * would at width H on this kernel.  Every entry is ONE launch, reads nothing on the host and is capturable.
 *   resel_gru_pad_params:   w_ih [3H, n_in], b_ih [3H], w_hh [3H, H], b_hh [3H] -> [3Hk, n_in], [3Hk], [3Hk, Hk], [3Hk].
 *                           w_ih / b_ih and their outputs may all four be NULL (n_in is then ignored): recurrent parameters only.
 *   resel_gru_unpad_params: the inverse slice, for the four gradients (same NULL rule).
 *   resel_gru_pad_rows:     src [rows, G, H] -> dst [rows, G, Hk], zero-filled (G = 3: gi; G = 1: h0, dh_all).  1 <= G <= 4.
 *   resel_gru_unpad_rows:   src [rows, G, Hk] -> dst [rows, G, H] (h_all, dgi).
 * RESEL_EINVAL: a NULL or not 4-byte aligned pointer, Hk not a supported kernel width, H outside 1 .. Hk - 1, n_in < 1, rows < 1,
 * G outside 1 .. 4, or a tensor of 2^31 elements or more. */
int resel_gru_pad_params(const float* w_ih, const float* b_ih, const float* w_hh, const float* b_hh,
                         float* w_ih_k, float* b_ih_k, float* w_hh_k, float* b_hh_k, int n_in, int H, int Hk, resel_stream_t stream);
int resel_gru_unpad_params(const float* dw_ih_k, const float* db_ih_k, const float* dw_hh_k, const float* db_hh_k,
                           float* dw_ih, float* db_ih, float* dw_hh, float* db_hh, int n_in, int H, int Hk, resel_stream_t stream);
int resel_gru_pad_rows(const float* src, float* dst, long long rows, int G, int H, int Hk, resel_stream_t stream);
int resel_gru_unpad_rows(const float* src, float* dst, long long rows, int G, int H, int Hk, resel_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * cgpt attention core: packed var-len causal attention with ALiBi, bf16 MFMA (v_mfma_f32_32x32x16_bf16), fp32 softmax.
 * Replaces the flash-attn varlen kernels reached through `flash_attn.modules.mha.MHA(causal=True, use_alibi=True)`
 * (offpolicy_rnn/models/flash_attention/TransformerFlashAttention.py:67-70, called under bf16 autocast at :80-81; packing
 * :107-112).  *** flash_attn is an un-vendored dependency: semantics restated (softmax(q k^T * scale - slope_h (i - j)), j <= i),
 * parity unpinned ***
 * qkv: [T, 3, H, hd] bf16 packed tokens (q | k | v); cu_seqlens: int32 [S + 1] device; slopes: [H] fp32 or NULL;
 * out: [T, H, hd] bf16; lse: [H, T] fp32 (base-2 log-sum-exp, saved for the backward).  hd in {32, 64, 128}; max_seqlen bounds
 * the grid.  Backward: dqkv [T, 3, H, hd] bf16 (fully overwritten); workspace resel_attn_varlen_bwd_workspace_bytes().
 * Forward workspace (resel_attn_varlen_fwd_workspace_bytes(), may be NULL): holds the device-built work list - the real
 * (sequence, 128-token block) items of the ragged batch, longest first - that the kernels' workgroups take their work from;
 * without it they run in (sequence, block) order, which is slower on ragged batches.  Results do not depend on it.
 * Attention-probability dropout (MHA(dropout=p), TransformerFlashAttention.py:67-70, active in .train() passes): p_drop in
 * [0, 1); the keep mask is a counter function of (seed, offset, head, packed query token, key position) - no state, the
 * backward regenerates it from the same (seed, offset).  8-bit keep threshold floor((1 - p) * 255) + 1 and the 1 / (1 - p)
 * rescale as in flash-attn; the counter function itself is this library's (oracle/kernels.py `attn_dropout_keep`).
 * p_drop == 0 runs the dropout-free kernels.
 */
size_t resel_attn_varlen_fwd_workspace_bytes(int S, int max_seqlen);
int resel_attn_varlen_fwd(const uint16_t* qkv, const int32_t* cu_seqlens, const float* slopes, uint16_t* out, float* lse,
                          void* workspace, int T, int S, int H, int hd, int max_seqlen, float scale,
                          float p_drop, uint64_t seed, uint64_t offset, resel_stream_t stream);
size_t resel_attn_varlen_bwd_workspace_bytes(int T, int S, int H, int hd, int max_seqlen);
int resel_attn_varlen_bwd(const uint16_t* qkv, const int32_t* cu_seqlens, const float* slopes, const uint16_t* out,
                          const float* lse, const uint16_t* dout, uint16_t* dqkv, void* workspace,
                          int T, int S, int H, int hd, int max_seqlen, float scale,
                          float p_drop, uint64_t seed, uint64_t offset, resel_stream_t stream);
/* Padded forms (sequence tables of a shape bucket, algorithm/graphed_update.py `seq_buckets`): same arguments, same kernels and
 * workspaces, but T may exceed cu_seqlens[S] and sequences may have length zero (cu_seqlens padded by repeating its last value).
 * Rows [0, cu_seqlens[S]) are bit for bit what the entries above give on the unpadded problem; rows [cu_seqlens[S], T) of out, of
 * every head's lse and of dqkv are written as zero by one more pass that reads the token count on the device and touches only
 * that tail (no whole-tensor memset) - inside a recorded graph's static pool they would otherwise hold stale bits. */
int resel_attn_varlen_fwd_padded(const uint16_t* qkv, const int32_t* cu_seqlens, const float* slopes, uint16_t* out, float* lse,
                                 void* workspace, int T, int S, int H, int hd, int max_seqlen, float scale,
                                 float p_drop, uint64_t seed, uint64_t offset, resel_stream_t stream);
int resel_attn_varlen_bwd_padded(const uint16_t* qkv, const int32_t* cu_seqlens, const float* slopes, const uint16_t* out,
                                 const float* lse, const uint16_t* dout, uint16_t* dqkv, void* workspace,
                                 int T, int S, int H, int hd, int max_seqlen, float scale,
                                 float p_drop, uint64_t seed, uint64_t offset, resel_stream_t stream);

/* Token packing with a DEVICE-side token count (padded sequence tables: idx has the bucket's length T, *n_dev = cu_seqlens[S] of
 * them are real).  fp32 rows of C floats, C % 4 == 0, 16-byte aligned bases, leading dimensions multiples of 4.
 *   pack:   out[t] = t < *n_dev ? src[idx[t]] : 0 for t < T  (what `index_select` does at a fixed size, plus a zero tail);
 *           idx[t] must be a row of src for t < *n_dev, the entries behind are never read.
 *   unpack: EVERY row m < M of dst is written exactly once per call: packed[t] where some t < *n_dev has idx[t] == m, zeros
 *           otherwise (what `zeros.index_copy` does, without a memset pass, without a write race, deterministic).  idx must be
 *           strictly increasing over [0, *n_dev) - a per-row binary search finds the source.
 * *n_dev is clamped to [0, T].  Each is the other's gradient (a padded token carries a zero gradient). */
int resel_pack_rows(const float* src, int64_t ld_src, const int64_t* idx, const int32_t* n_dev, float* out, int64_t ld_out,
                    int T, int C, resel_stream_t stream);
int resel_unpack_rows(const float* packed, int64_t ld, const int64_t* idx, const int32_t* n_dev, float* dst, int64_t ld_dst,
                      int M, int T, int C, resel_stream_t stream);

/* Head-width padding around the attention entries.  The kernels above and resel_attn_decode exist for hd in {32, 64, 128}; every other
 * multiple of 8 up to 120 runs on the next of these widths hdp (8..24 -> 32, 40..56 -> 64, 72..120 -> 128): zero columns of q and k add
 * nothing to a score and zero columns of v give zero output columns, so the result is exact as long as `scale` is that of the TRUE
 * width.  bf16 rows of hd resp. hdp elements, both multiples of 8, hdp >= hd, 16-byte aligned bases, dense tensors.
 *   pad:   src [T, n, H, hd] -> dst [T, n, H, hdp], columns [hd, hdp) written as zero   (qkv: n = 3; dout: n = 1)
 *   unpad: src [T, n, H, hdp] -> dst [T, n, H, hd], the first hd columns of every row   (out: n = 1; dqkv: n = 3)
 * Every element of dst is written exactly once.  No host read, no allocation: capturable.  hdp == hd is a plain copy. */
int resel_head_pad(const uint16_t* src, uint16_t* dst, int T, int n, int H, int hd, int hdp, resel_stream_t stream);
int resel_head_unpad(const uint16_t* src, uint16_t* dst, int T, int n, int H, int hd, int hdp, resel_stream_t stream);

/* Element-wise dropout y = keep(i) ? x / (1 - p) : 0 with the keep mask a counter function of (seed, offset, element index)
 * (16-bit threshold round((1 - p) * 65536); oracle/kernels.py `dropout_keep`).  Replaces the `nn.Dropout`s of the cgpt
 * decoder block (TransformerFlashAttention.py:48,52,72,84-85) in training-mode passes; the backward is the same call on dy
 * with the same (seed, offset).  In place (y == x) allowed. */
int resel_dropout(const float* x, float* y, int64_t n, float p_drop, uint64_t seed, uint64_t offset, resel_stream_t stream);
/* Offset base of the counter-keyed masks: while `base` (a device uint64, 8-byte aligned; NULL switches it off) is set, every mask
 * kernel launched afterwards - resel_dropout, resel_gelu_dropout_fwd / _bwd, resel_attn_varlen_fwd / _bwd with p_drop > 0 - adds
 * *base to its `offset` argument WHEN IT RUNS.  A captured update (algorithm/graphed_update.py) bakes the host-drawn offsets into
 * its kernel nodes; a node of the same graph advances *base, so every replay draws fresh masks while the forward and backward
 * kernels of one replay agree.  Process-wide host state (one device per process); not a per-call argument. */
int resel_dropout_offset_base(const void* base);
/* y = dropout(gelu(x)) (erf form) in one pass and its backward dx = dy * keep / (1 - p) * gelu'(x) from the pre-activation x; same
 * counter-keyed mask as resel_dropout (p_drop = 0: plain GELU).  FFN hidden of the cgpt block (reference
 * models/flash_attention/TransformerFlashAttention.py:46-53: nn.GELU() followed by nn.Dropout). */
int resel_gelu_dropout_fwd(const float* x, float* y, int64_t n, float p_drop, uint64_t seed, uint64_t offset,
                           void* amax_y, unsigned amax_epoch, resel_stream_t stream);
int resel_gelu_dropout_bwd(const float* x, const float* dy, float* dx, int64_t n, float p_drop, uint64_t seed, uint64_t offset,
                           void* amax_dx, unsigned amax_epoch, resel_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * SAC / TD3 head, target and loss arithmetic + optimizer tail (the "fusions" of SURVEY.md section 8 row a16-a18).
 */
/* tanh-Gaussian head: contextual_sac_policy_single_head.py:109-123.  out2: [M, 2A] = (logstd | mean) as produced
 * by the actor's last Linear; noise: [M, A].  action_mean, action_sample: [M, A]; logp: [M].
 * Backward: d_out2 [M, 2A] from d_sample [M, A] and d_logp [M] (action_mean carries no gradient in the update). */
int resel_tanh_gaussian_fwd(const float* out2, const float* noise, float* action_mean, float* action_sample,
                            float* logp, int M, int A, resel_stream_t stream);
int resel_tanh_gaussian_bwd(const float* out2, const float* noise, const float* d_sample, const float* d_logp,
                            float* d_out2, int M, int A, resel_stream_t stream);

/* REDQ target: sac_full_length_rnn_redq.py:28-33 / td3_full_length_rnn_redq.py:29-35, clamp = QValueGuard
 * (utility/q_value_guard.py:22-38).  q: [E, M]; subset: m ensemble indices; next_logp: [M] or NULL (TD3);
 * done (already timeout-corrected), reward, mask: [M].  guard: device fp32[4] = {min, max, initialised, decay}:
 *   if !initialised: min/max <- extrema of v (first call, q_value_guard.py:23-26);  y = r + (1-d) gamma clamp(v)
 *   then the running update of q_value_guard.py:29-38 with y*mask - all on device, no host sync.
 * target: [M].  stats (optional) fp32[2]: max |target|, sum(mask).
 * NaN: a NaN in a SELECTED member's next-Q (or in next_logp) makes target[i] NaN, as q.min(dim=0) and clamp of the reference
 * do, so that the critic loss shows it.  The guard does not follow the reference there (its .item() extrema would turn NaN for
 * good): the extrema behind the first-call initialisation, the running update and stats[0] are taken with fminf / fmaxf and
 * skip NaN elements, so the guard keeps describing the finite rows of the batch.  A batch without a single finite row has the
 * extrema {+inf, -inf}: it leaves an initialised guard as it is at decay 1 and makes it infinite at a decay below 1.  The same
 * holds for the data-parallel forms below. */
int resel_sac_target(const float* q, const int32_t* subset, int m, const float* next_logp, const float* log_alpha,
                     const float* reward, const float* done, const float* mask, float gamma, float* guard,
                     float* target, float* stats, void* workspace, int E, int M, resel_stream_t stream);
/* The same target in three phases for data-parallel runs: the Q-guard of the reference sees the extrema of the WHOLE batch
 * (utility/q_value_guard.py:22-38), so between the phases the caller all-reduces (MAX) the two-float blocks of `extrema`
 * [4] = {-min v, max v, -min(y mask), max(y mask)}: phase 0 writes [0:2] (rank-local), phase 1 initialises the guard from
 * the (now global) [0:2], clamps, forms y and writes [2:4], phase 2 updates the guard from the (now global) [2:4].
 * Same workspace for all phases of one target. */
int resel_sac_target_phase(int phase, const float* q, const int32_t* subset, int m, const float* next_logp, const float* log_alpha,
                           const float* reward, const float* done, const float* mask, float gamma, float* guard,
                           float* target, float* stats, float* extrema, void* workspace, int E, int M, resel_stream_t stream);
/* Data parallel with ONE collective per optimizer step (north_star: "a RCCL all-reduce of gradients ... and no other collectives"):
 * resel_sac_target_local forms the target from the rank's own rows with the guard AS IT STANDS (an uninitialised guard does not
 * clamp - on one process its first interval is the batch's own range, so the first clamp is the identity there too) and writes
 * the rank-local extrema [4] = {-min v, max v, -min(y mask), max(y mask)}; the caller puts them into its own row of a zero-filled
 * [world][4] tail of the critic gradient bucket, and after the SUM all-reduce resel_guard_apply_slots initialises / updates the
 * guard from the maxima over the rows - the guard of update k + 1 is then the one a single process over the global batch has
 * (the guard of the reference acts on the NEXT target only: utility/q_value_guard.py:22-38). */
int resel_sac_target_local(const float* q, const int32_t* subset, int m, const float* next_logp, const float* log_alpha,
                           const float* reward, const float* done, const float* mask, float gamma, const float* guard,
                           float* target, float* stats, float* extrema, void* workspace, int E, int M, resel_stream_t stream);
int resel_guard_apply_slots(const float* slots, int world, float* guard, resel_stream_t stream);
size_t resel_sac_target_workspace_bytes(int M);
/* The target of the memoryless REDQ trainer (reference algorithm/sac_mlp_redq_ensemble_q.py:29-39): no Q-guard and no mask.
 *   target[i] = reward[i] + (1 - done[i]) gamma (min_{e in subset} q[e][i] - exp(log_alpha) next_logp[i]),  stats[0] = max_i |target[i]|
 * q [E][M]; subset [m] int32 on the device, entries clamped into [0, E); next_logp NULL drops the entropy term; stats NULL: the
 * maximum is not formed.  A NaN member makes its minimum NaN.  workspace: resel_sac_target_workspace_bytes(M) bytes. */
int resel_redq_target(const float* q, const int32_t* subset, int m, const float* next_logp, const float* log_alpha,
                      const float* reward, const float* done, float gamma, float* target, float* stats, void* workspace,
                      int E, int M, resel_stream_t stream);

/* Masked losses of the update, one forward and one backward pass each (reference sac_full_length_rnn_ensembleQ.py:80-81 `_mask_mean`,
 * :105-114 `_Q_loss`, sac_full_length_rnn_redq.py:37-49 / td3_full_length_rnn_redq.py:39-51 `_policy_loss`, :130-132 `_alpha_loss`);
 * UN-normalised sums (the global valid count divides the gradient inside AdamW).  q [E][M], y / mask / logp [M] (mask NULL = ones).
 *   critic  out2[0] = sum_m mask sum_e (q - y)^2;                           dq = 2 g[0] mask (q - y)
 *   actor   out2[0] = sum_m mask (use_logp exp(log_alpha) logp - red_e q),  out2[1] = sum_m mask logp;   red = mean (reduce_min 0) / min (1)
 *           dlogp = g[0] exp(log_alpha) mask;  dq = -g[0] mask / E (mean)  or  -g[0] mask at the FIRST minimal member, 0 elsewhere (min)
 * g: device scalar (the incoming gradient of the sum).  Fixed-order two-stage sums; workspace: resel_masked_loss_workspace_bytes(). */
size_t resel_masked_loss_workspace_bytes(void);
int resel_q_loss_fwd(const float* q, const float* y, const float* mask, float* out2, void* workspace, int E, int M, resel_stream_t stream);
int resel_q_loss_bwd(const float* q, const float* y, const float* mask, const float* g, float* dq, int E, int M, resel_stream_t stream);
int resel_actor_loss_fwd(const float* logp, const float* q, const float* mask, const float* log_alpha, float* out2, void* workspace,
                         int E, int M, int use_logp, int reduce_min, resel_stream_t stream);
int resel_actor_loss_bwd(const float* q, const float* mask, const float* log_alpha, const float* g, float* dlogp, float* dq,
                         int E, int M, int use_logp, int reduce_min, resel_stream_t stream);

/* Flat-buffer optimizer tail.  All parameter / gradient / moment tensors of one network live in ONE fp32 buffer.
 * soft update: rnn_base.py:490-491   target <- tau * target + (1 - tau) * online
 * adamw: torch.optim.AdamW (sac.py:61) with a per-segment learning rate table (RESeL groups,
 *        sac_full_length_rnn_redq_sep_optim.py:49-66): seg_end[i] = one-past-last element of segment i,
 *        seg_lr[i], seg_wd[i]; grad_scale multiplies the gradient first (1/valid_num or 1/world).
 * sumsq: out[0] = sum(x^2)  (l2_norm_square, rnn_base.py:531-532), deterministic two-stage reduction. */
int resel_soft_update(float* target, const float* online, float tau, int64_t n, resel_stream_t stream);
int resel_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end,
                     const float* seg_lr, const float* seg_wd, int nseg, float beta1, float beta2, float eps,
                     int step, const float* grad_scale, resel_stream_t stream);
/* The same step with the step-dependent factors taken BY VALUE: bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t) as the caller formed
 * them.  The eager update passes the values FlatAdamW.prepare_step() writes for the captured one (fp64 on the host, rounded once), so
 * that an eagerly launched and a replayed update take bit-identical steps; resel_adamw_flat forms them in fp32 from `step`, where
 * 1 - beta2^t loses up to 6e-5 / t of its value to cancellation. */
int resel_adamw_flat_bc(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end,
                        const float* seg_lr, const float* seg_wd, int nseg, float beta1, float beta2, float eps,
                        float bc1, float bc2_sqrt, const float* grad_scale, resel_stream_t stream);
/* The same step with the step-dependent factors read from DEVICE memory: bias_corrections[0] = 1 - beta1^t,
 * bias_corrections[1] = sqrt(1 - beta2^t).  For updates replayed from a hipGraph, where a by-value step would be frozen at capture. */
int resel_adamw_flat_dev(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end,
                         const float* seg_lr, const float* seg_wd, int nseg, float beta1, float beta2, float eps,
                         const float* bias_corrections, const float* grad_scale, resel_stream_t stream);
size_t resel_sumsq_workspace_bytes(int64_t n);
int resel_sumsq(const float* x, int64_t n, float* out, void* workspace, resel_stream_t stream);

/* ---- bias + activation tail of fc / efc-E layers, fused around the library GEMM -------------------------------
 * Replaces `activation(linear(x))` of reference models/rnn_base.py:462-474 (nn.Linear / EnsembleLinear followed by the
 * per-layer activation module) for act = ELU, and the bias add of EnsembleLinear (ensemble_linear_model.py:60-67).
 * y [rows, C] contiguous, rows grouped in rows / rows_per_seg segments with one bias row [C] each (bias [nseg, C]).
 * fwd (in place): y <- act(y + bias);  act: 0 = identity, 1 = ELU(alpha = 1), and the other activations of the reference's ACTIVATIONS
 *      table that are derivable from their output (no ABI change: codes the entries used to refuse):
 *          code  activation                        act'(.) from the output a
 *            6   relu        max(v, 0)             a > 0 ? 1 : 0
 *            7   leaky_relu  v > 0 ? v : 0.01f v   a > 0 ? 1 : 0.01     (torch's default slope; an fp32 product: torch's bits)
 *            8   tanh                              1 - a^2              (v_exp / v_rcp; tanh(+-0) = +-0, exactly +-1 past |v| = 44)
 *            9   sigmoid                           a (1 - a)            (exactly 0 below v = -88.8, exactly 1 above 17.4)
 *      Any other code (2 .. 5 belong to the GEMM entries) is RESEL_EINVAL before anything is enqueued.
 * bwd (from the forward OUTPUT a): gy = g * act'(.), dbias[nseg, C] = per-segment column sums of gy (dbias may be NULL).  g has row
 *      stride ldg >= C (a column block of a wider gradient is read in place: ABI 7), a has row stride lda >= C (a block of a row buffer
 *      that its producing GEMM wrote in place: ABI 8), gy is dense; gy NULL with act == 0 = column sums only.
 *      workspace: resel_bias_act_bwd_workspace_bytes. */
int resel_bias_act_fwd(float* y, const float* bias, int64_t rows, int C, int64_t rows_per_seg, int act, resel_stream_t stream);
size_t resel_bias_act_bwd_workspace_bytes(int64_t rows, int C, int64_t rows_per_seg);
int resel_bias_act_bwd(const float* g, int64_t ldg, const float* a, int64_t lda, float* gy, float* dbias, void* workspace, int64_t rows, int C,
                       int64_t rows_per_seg, int act, void* amax_gy, unsigned amax_epoch, resel_stream_t stream);

/* ---- ensemble head: last hidden layer's tail + the width-1 output layer of an efc-E MLP ----------------------------
 * The critic head of the reference is `efc-E(H) ELU -> efc-E(1)` (policy_value_models/contextual_sac_value.py via
 * models/rnn_base.py:462-474; EnsembleLinear weight [E, H, 1], bias [E, 1, 1]).  y [E*M, H] is the hidden layer's GEMM output.
 * fwd: a = elu(y + b2[e]) in place, q[e*M + m] = sum_c a[c] * w3[e, c] + b3[e]          (b2, w3: [E, H]; b3: [E] or NULL)
 * bwd: gy = gq[r] * w3[e] * elu'(a), db2[E, H] = sum_m gy, dw3[E, H] = sum_m a * gq     (db3 = sum_m gq is left to the host) */
int resel_ensemble_head_fwd(float* y, const float* b2, const float* w3, const float* b3, float* q, int64_t rows, int H,
                            int64_t rows_per_seg, resel_stream_t stream);
size_t resel_ensemble_head_bwd_workspace_bytes(int64_t rows, int H, int64_t rows_per_seg);
int resel_ensemble_head_bwd(const float* gq, const float* a, const float* w3, float* gy, float* db2, float* dw3, void* workspace,
                            int64_t rows, int H, int64_t rows_per_seg, void* amax_gy, unsigned amax_epoch, resel_stream_t stream);

/* ---- fp32 GEMM on the matrix cores, tails fused --------------------------------------------------------------------------
 * C[b][m][n] = act( sum_k A[b](m, k) B[b](n, k) + bias[b][n] ),  b < batch (ensemble member; strides in floats).
 * An operand is a [rows][K] matrix (x_kcontig = 1: activations, nn.Linear / EnsembleLinear weights [out][in]) or a [K][rows]
 * matrix (x_kcontig = 0: the transposed use of an activation matrix in a weight gradient, of a weight in an input gradient):
 *   forward  y = x W^T (+ bias, ELU)   A = x  (1), B = W (1)      torch.nn.Linear (models/rnn_base.py:101-105),
 *   dgrad    dx = dy W                 A = dy (1), B = W (0)      EnsembleLinear (models/ensemble_linear_model.py:36-49)
 *   wgrad    dW = dy^T x               A = dy (0), B = x (0)      K = number of tokens: split over blocks, partial tiles summed in
 *                                                                  a fixed order (workspace: resel_gemm_f32_workspace_bytes)
 * act: 0 none, 1 ELU, 2 accumulate (C += product + bias: the accumulating form of an input gradient; no activation), 3 softplus (resel_gemm_f32x only),
 *      6 relu, 7 leaky_relu (slope 0.01), 8 tanh, 9 sigmoid: the code table of resel_bias_act_fwd, in every plain epilogue (the third edition
 *      compiles them as an instantiation of its own); amax_c is the magnitude of the stored, activated values, as for ELU.  4 / 5 are the fused
 *      entries' (resel_gemm_f32_dact / _head: ELU only) and are refused here, like anything else.
 * EVERY extent and alignment is taken (round 6; no ABI change): the matrix-core kernels need the contiguous extent of each operand (K or rows) to be a
 * multiple of 4, 16-byte aligned rows and row strides < 2^22; operands that are not - the 6-wide TD3 / discrete heads and their gradients, a rank-2
 * dt_proj, odd action counts - and the M <= 8 rows of a rollout step against a whole weight matrix (models/rnn_base.py single-step branch,
 * smamba/mamba.py:257-305) run csrc/gemm_any.hip: exact fp32 FMAs, the same epilogues, the same magnitude publication, long reductions cut in
 * K and summed in a fixed order.  No call of this entry is left to a vendor library by the host side (tests/test_no_library_gemm_gpu.py).
 * split selects how the fp32 products are formed (inputs, accumulation and outputs are fp32 in every mode):
 *   0  v_mfma_f32_32x32x2_f32 (fp32 operands, exact products);
 *   6  each operand split EXACTLY into three bf16 planes (8 + 8 + 8 significant bits), the six leading plane products - each exact -
 *      accumulated in fp32 by v_mfma_f32_32x32x16_bf16 (the three dropped terms are each <= 2^-24 |a b|, the size of one fp32 rounding
 *      of the product);
 *   3  "bf16x3": two planes per operand (16 significant bits) and the three leading plane products; every dropped term is
 *      <= 2^-16 |a b|.  The class torch names float32 matmul precision 'high' (TF32 / bf16x3) - NOT the reference's default
 *      ('highest' = modes 0 / 2 / 6); half the matrix instructions of mode 6.  Shapes with M <= 128 run mode 6;
 *   2  see resel_gemm_f32x below.
 * (Modes 9 - all nine plane products - and 106 / 109 - modes 6 / 9 on the first-edition kernel - were A/B forms of rounds 2-4; removed
 * in ABI 7.)  Mode 6 splits each operand element once per block on its way into LDS (csrc/gemm_bf3.hip, 256 x 128 tiles); M <= 128
 * takes the first-edition kernel of csrc/gemm_f32.hip (128 x 128 tiles, every wave splits the fragments it reads). */
size_t resel_gemm_f32_workspace_bytes(int M, int N, int K, int batch);
int resel_gemm_f32(const float* A, int64_t lda, int64_t strideA, int a_kcontig,
                   const float* B, int64_t ldb, int64_t strideB, int b_kcontig,
                   const float* bias, int64_t strideBias, int act,
                   float* C, int64_t ldc, int64_t strideC, void* workspace,
                   int M, int N, int K, int batch, int split, resel_stream_t stream);

/* Mode 2 ("f16x3") of the same contract: fp16 planes of the SCALED operands, three plane products on v_mfma_f32_32x32x16_f16,
 * one fp32 accumulator - half the matrix instructions of mode 6.  Each operand is multiplied by a power of two s that brings its
 * largest magnitude into [2^14, 2^15), then A -> a1 = fp16(x s), a2 = fp16(2^11 (x s - a1)); B -> b1 = fp16(x s),
 * b2 = fp16(x s - b1), b1s = 2^-11 b1;  C = (a1 b1 + a1 b2 + a2 b1s) / (sA sB).  The residuals and the plane products are exact in
 * fp32; the dropped term is <= 2^-22 |a b|.  Every element of A keeps 22 significant bits down to 2^-29 max|A|, of B down to
 * 2^-18 max|B| (below: 40 - log2(max|B| / |x|) bits) - pass the weights (forward, input gradient) or the narrower-range operand
 * as B.  Error against fp64 <= the fp32 instruction's for A over 12 decades and B over 6 (tools/eval_f16_split.py,
 * tests/test_hip_ops.py::test_gemm_f32_f16x3_mode_error_against_fp64).  amax_a / amax_b: magnitude HANDLES (below) holding an upper bound of
 * max |A| / max |B| over the whole operand (all batch members) - resel_amax, or what the producer of the operand published; a
 * bound 2^k too large costs k bits of those ranges, one too small overflows fp16 (inf in C).  Other modes ignore the two pointers
 * (may be NULL).  M <= 128 and K < 32 fall back to modes 6 / 0.
 * Two kernels serve mode 2 (same results to rounding of the same three plane products; b1s is formed from b1 next to the matrix
 * instruction in both): the producer / consumer edition for K and K slices that are multiples of 32 and row strides < 2^22
 * (csrc/gemm_bf3.hip `gemm_ws_kernel`), the one-role edition (`gemm_bf3_kernel`) for the rest: the shape alone decides. */
int resel_gemm_f32x(const float* A, int64_t lda, int64_t strideA, int a_kcontig,
                    const float* B, int64_t ldb, int64_t strideB, int b_kcontig,
                    const float* bias, int64_t strideBias, int act,
                    float* C, int64_t ldc, int64_t strideC, void* workspace,
                    int M, int N, int K, int batch, int split, const float* amax_a, const float* amax_b,
                    void* amax_c, unsigned amax_epoch, resel_stream_t stream);
/* Fused epilogues of the producer / consumer edition (ABI 7).  Product mode 2 only (magnitude handles required), K a multiple of 32,
 * M > 128, row strides < 2^22; dact also needs M >= 256 and N a multiple of 128 (rows past the last whole 256-row tile take the plain
 * product + one small in-place pass inside the call) - resel_gemm_f32_fused_supported(kind, ...) says whether a shape qualifies; operand
 * layouts as resel_gemm_f32, A in its [rows][K] form.
 * Both write per-wave partial reductions into `workspace` (resel_gemm_f32_fused_workspace_bytes(M, N, K, batch, kind); kind 4 = dact,
 * 5 = head) and fold them with a second small kernel in a fixed order: deterministic, no atomics.
 *
 * resel_gemm_f32_dact - the input gradient of a layer whose input is the ELU output Y of the layer below, with that ELU's derivative and
 *   that layer's bias gradient in the epilogue (reference: rnn_base.py:461-469 applies the activation module after every fc / efc layer;
 *   autograd runs elu_backward and the bias sum as separate passes):
 *     C[b][m][n] = (sum_k A[b](m, k) B[b](n, k)) * (Y[b][m][n] > 0 ? 1 : Y[b][m][n] + 1);   dbias[b][n] = sum_m C[b][m][n]  (dbias may be NULL)
 *   Y: row stride ldy, batch stride strideY, same [m][n] indexing as C.
 * resel_gemm_f32_head - the last two layers of an efc-E critic head (reference ensemble_linear_model.py:36-49 via rnn_base.py:421-469:
 *   efc-E(H) -> ELU -> efc-E(1)) in one GEMM:
 *     C[b][m][n] = a = elu(sum_k A[b](m, k) B[b](n, k) + bias[b][n]);   q[b][m] = sum_n a[b][m][n] w3[b][n] + b3[b]  (b3 may be NULL)
 *   (C is kept: the backward needs the hidden activation). */
int resel_gemm_f32_fused_supported(int kind, int M, int N, int K, int64_t lda, int64_t ldb);
size_t resel_gemm_f32_fused_workspace_bytes(int M, int N, int K, int batch, int kind);
int resel_gemm_f32_dact(const float* A, int64_t lda, int64_t strideA, int a_kcontig,
                        const float* B, int64_t ldb, int64_t strideB, int b_kcontig,
                        const float* Y, int64_t ldy, int64_t strideY,
                        float* C, int64_t ldc, int64_t strideC, float* dbias, void* workspace,
                        int M, int N, int K, int batch, const float* amax_a, const float* amax_b,
                        void* amax_c, unsigned amax_epoch, resel_stream_t stream);
int resel_gemm_f32_head(const float* A, int64_t lda, int64_t strideA, int a_kcontig,
                        const float* B, int64_t ldb, int64_t strideB, int b_kcontig,
                        const float* bias, int64_t strideBias, const float* w3, int64_t strideW3, const float* b3,
                        float* C, int64_t ldc, int64_t strideC, float* q, void* workspace,
                        int M, int N, int K, int batch, const float* amax_a, const float* amax_b,
                        void* amax_c, unsigned amax_epoch, resel_stream_t stream);
/* out [rows, cols] (row stride ld_out) = zeros with nblk <= 8 source blocks copied in: block k = src[k] [nr[k], nc[k]] (row stride ld_src[k]) placed
 * at (r0[k], c0[k]); later blocks win where blocks overlap.  The arrays are HOST arrays of length nblk (read before the call returns).  One launch
 * for the operands of the merged input-encoder GEMM - the block-diagonal of the encoder weights, their concatenated biases, the concatenated
 * zero-padded input rows (reference contextual_sac_value.py:90-99 / contextual_sac_policy.py: one nn.Linear per input and a cat of the outputs).
 * (ABI 8) */
int resel_place_blocks(float* out, int64_t ld_out, int rows, int cols, int nblk, const float* const* src, const int64_t* ld_src,
                       const int* r0, const int* nr, const int* c0, const int* nc, resel_stream_t stream);

/* Magnitude handles.  A kernel that writes a tensor which a later GEMM reads can publish max |x| of what it stored, so that mode 2
 * needs no extra pass over the operand.  A handle is 1 KiB (8-byte aligned; NULL = off): eight 8-byte words 128 bytes apart, word j =
 * {float bits : low 32 | epoch : high 32}; a publishing wave raises the word its workgroup id selects with one 64-bit atomicMax
 * (eight lines: thousands of waves finishing together would serialise on one).  A larger epoch outranks any older content - handles
 * are never zeroed, give every tensor a fresh epoch - and kernels that fill parts of one tensor may share handle and epoch.  Readers
 * (amax_a / amax_b above) take the newest epoch among the eight words and the largest magnitude carrying it.  Publishers:
 * resel_amax (a pre-pass), resel_gemm_f32x (amax_c: the values stored to C), resel_bias_act_bwd (gy), resel_ensemble_head_bwd (gy), resel_add_layernorm_fwd
 * (y: the analytic bound sqrt(C) max|w| + max|b|, published by one wave), resel_add_layernorm_bwd (dx), resel_member_layernorm_fwd / _bwd (likewise), resel_selective_scan_fwd (out), resel_selective_scan_bwd (dz, ddelta),
 * resel_causal_conv1d_fwd (y), resel_causal_conv1d_bwd (dx), resel_gelu_dropout_fwd / _bwd (y / dx). */
/* Magnitude pre-pass: max |x| over a [batch][rows][cols] box (row stride ld, batch stride `stride`, cols % 4 == 0) written into the
 * magnitude handle `out` with epoch `epoch` (see "magnitude handles" above); one HBM-bound pass, no host synchronisation.
 * The call keeps no state: any number of pre-passes may be in flight on any streams (a maximum is order-independent, every wave raises
 * the handle with one conditional atomicMax).  `state` is ignored (may be NULL) and resel_amax_state_bytes() returns 0 since ABI 7; both
 * stay in the signature so that ABI 6 callers keep linking. */
/* Magnitudes of every tensor of a flat parameter buffer in ONE launch: segment g = flat[begin[g], begin[g] + len[g]) (device int64
 * tables) publishes into the g-th of `nseg` consecutive 1 KiB handles at `handles` under `epoch` (the weights change once per optimizer
 * step / soft update; the GEMMs of the update then find their weight's magnitude without a pre-pass per call). */
int resel_amax_segments(const float* flat, const int64_t* begin, const int64_t* len, int nseg, void* handles, unsigned epoch,
                        resel_stream_t stream);
size_t resel_amax_state_bytes(void);
int resel_amax(const float* x, int64_t ld, int64_t stride, int rows, int cols, int batch, void* out, unsigned epoch, void* state,
               resel_stream_t stream);
/* Verify mode (ABI 7): does `handle` hold an upper bound of max |x| over the same box?  Waves whose maximum exceeds it report into the
 * device words err[0..3] (int32, zero = clean): [0] reporting waves, [1] float bits of the largest violating magnitude, [2] `tag` (!= 0)
 * of the first report, [3] float bits of the bound it saw.  No host synchronisation; the caller reads `err` when it wants the verdict.
 * The Python side runs it in front of every mode-2 product when RESEL_AMAX_VERIFY=1 (hip/ops.py `amax_verify_raise`). */
int resel_amax_check(const float* x, int64_t ld, int64_t stride, int rows, int cols, int batch, const void* handle, int* err, int tag,
                     resel_stream_t stream);

/* ---- mixed-precision GEMM for the bf16 attention projections (cgpt) ------------------------------------------------------
 * C[m][n] = sum_k bf16(A(m, k)) bf16(B(n, k)) + bf16(bias[n]): operands rounded to bf16 (round to nearest even) on their way
 * into LDS, fp32 accumulation (v_mfma_f32_32x32x16_bf16), C stored as bf16 (c_bf16 = 1), as fp32 (0), or as fp32 holding the
 * bf16-rounded value (2: the autocast's rounding point without the cast pass that follows it).  A / B are fp32 or bf16 in
 * memory (x_bf16) and [rows][K] (x_kcontig = 1) or [K][rows]; lda / ldb / ldc in ELEMENTS; bias fp32 or NULL.  This is what
 * F.linear computes under the reference's bf16 autocast (flash-attn MHA, TransformerFlashAttention.py:67-70) without the
 * separate cast passes: forward (A = activations, B = weight [N][K]), input gradient (B = weight as [K][rows]), weight
 * gradient (both operands [K = tokens][rows]; K slices summed in a fixed order, workspace: resel_gemm_bf16_workspace_bytes).
 * The matrix-core kernel needs the contiguous extent of each operand to be a multiple of 4, leading dimensions multiples of 4 and bases 16-byte
 * (fp32) or 8-byte (bf16) aligned; other fp32 operands, and M <= 8 rows against a [N][K] fp32 weight (the decode step of flash-attn's MHA; A fp32 or
 * bf16), run csrc/gemm_any.hip with the same rounding points (round 6; no ABI change). */
size_t resel_gemm_bf16_workspace_bytes(int M, int N, int K);
int resel_gemm_bf16(const void* A, int64_t lda, int a_kcontig, int a_bf16, const void* B, int64_t ldb, int b_kcontig, int b_bf16,
                    const float* bias, void* C, int64_t ldc, int c_bf16, void* workspace, int M, int N, int K,
                    resel_stream_t stream);

/* Bias gradient of such a projection: out[n] = sum_m x[m][n] in fp32 for a bf16 matrix (row stride ld elements, ld % 8 == 0, N % 8 == 0,
 * N <= 2048, 16-byte aligned base) - the `gy.sum(0)` of the reference's autocast nn.Linear backward (TransformerFlashAttention.py:67-70
 * through flash-attn's MHA).  Fixed summation order (per-256-row partials, then their sum): bitwise reproducible. */
size_t resel_colsum_bf16_workspace_bytes(int M, int N);
int resel_colsum_bf16(const uint16_t* x, int64_t ld, int M, int N, float* out, void* workspace, resel_stream_t stream);

/* ---- packed trajectory batch from a device-resident replay ring --------------------------------------------------
 * Device counterpart of NestedMemoryArray.sample_trajs' packing loop (reference buffers/transition_buffer/
 * nested_replay_memory.py:140-176) plus the trainer's flag surgery (algorithm/sac_full_length_rnn_ensembleQ.py:338-342).
 * buffer [capacity, W] fp32 ring; segments [nseg][4] int32 = (batch row, first slot, length incl. `skip` leading slots,
 * first transition index) - the host-side sampling plan; pre_pairs [npairs][2] = (dst column, src column) of the pre-step
 * slot (next_state <- state, reward <- reward_input, state <- last_state of the trajectory's first transition).
 * out [rows, Tp, W + 3]: the W field columns, then validity, the target pass's validity and start flags.
 * A plan entry that does not fit (row >= rows, slot range beyond Tp, transitions beyond `capacity`) is dropped. */
int resel_gather_trajs(const float* buffer, int W, int64_t capacity, const int* segments, int nseg, int max_len, int skip, int rows, int Tp,
                       int c_mask, int c_start, int c_done, int c_timeout, const int* pre_pairs, int npairs,
                       float* out, resel_stream_t stream);
/* The same gather with a SELECTION of loss positions (randomised loss masks, reference nested_replay_memory.py:165-168: the host
 * draws which positions of each sampled trajectory keep their loss mask and ships the result with the plan).
 * sel [sel_words] int32 = [off_0 ... off_{nseg-1} | bitmap words]: off_s is the index of segment s's first bitmap word relative
 * to the start of the words part; bit (p & 31) of word off_s + (p >> 5) is 1 where data position p (0 ... length - skip - 1) of
 * segment s keeps its stored mask and 0 where its mask column becomes 0.  The validity column (W) receives the stored mask either
 * way.  A dropped plan entry never reads `sel`; a segment whose bitmap would reach outside the sel_words - nseg words keeps all
 * its masks.  sel == NULL: exactly the gather above (which forwards here).  sel_words < nseg is RESEL_EINVAL. */
int resel_gather_trajs_sel(const float* buffer, int W, int64_t capacity, const int* segments, int nseg, int max_len, int skip, int rows, int Tp,
                           int c_mask, int c_start, int c_done, int c_timeout, const int* pre_pairs, int npairs,
                           const int* sel, int sel_words, float* out, resel_stream_t stream);
/* Transition batches from the same ring (the memoryless trainers; reference replay_memory.py `sample_transitions`):
 *   out[n][:] = buffer[rows[p][n]][:]  for n < batch, all W columns;  out [batch][W], rows [passes][batch] int32.
 * p is the argument, or pass_word[0] when pass_word is not NULL (a device word: one captured launch then serves every pass of an update).
 * c_timeout >= 0: the done column of a row whose timeout column is > 0 is written as 0 (time-limit terminations bootstrap); -1 leaves
 * done as stored.  A row index outside [0, capacity), or a pass word outside [0, passes), yields a zero row and reads nothing of the
 * ring.  No alignment beyond 4 bytes and no multiple is asked of W or batch.  p outside [0, passes) without a pass word is RESEL_EINVAL. */
int resel_gather_transitions(const float* buffer, int W, int64_t capacity, const int* rows, int passes, int batch, int p,
                             const int* pass_word, int c_done, int c_timeout, float* out, resel_stream_t stream);
/* Slice batches from the same ring (the slice trainer; reference replay_memory_tail_padding.py `sample_fix_length_sub_trajs`), ONE launch:
 *   plan [passes][batch][2] int32 = (row0: ring row of the slice's first transition, n: its valid rows, 1 <= n <= L);
 *   out [batch][L + 1][W]:  slot 0      the PRE-STEP row: zero, except out[b][0][dst] = buffer[row0][src] for the npairs (dst, src) column
 *                                       pairs of pre_pairs (the convention of resel_gather_trajs; the slice trainer passes next_state <- state,
 *                                       state <- last_state, action <- last_action, reward <- reward_input);
 *                           slots 1..n  buffer[row0 .. row0 + n - 1][:], done written as 0 where the row's timeout column is > 0 (c_timeout >= 0);
 *                           slots n+1..L zero (the tail behind the trajectory's end: mask = 0).
 * out[:, 1:] is the batch, out[:, :] read through the destination columns is the L + 1 window of the target pass.  Every element of out
 * is written.  p is the argument, or pass_word[0] when pass_word is not NULL.  A plan entry with row0 < 0, n < 1, n > L or
 * row0 + n > capacity, or a pass word outside [0, passes), yields an all-zero slice and reads nothing of the ring; a pair whose source
 * column is outside [0, W) is skipped.  No alignment beyond 4 bytes and no multiple is asked of W, L or batch.  p outside [0, passes)
 * without a pass word, or (L + 1) * W above 65535 * 256, is RESEL_EINVAL. */
int resel_gather_slices(const float* buffer, int W, int64_t capacity, const int* plan, int passes, int batch, int L, int p,
                        const int* pass_word, int c_done, int c_timeout, const int* pre_pairs, int npairs, float* out, resel_stream_t stream);

/* ---- one-token rollout step (T = 1): the policy forward between updates -------------------------------------------
 * Reference: the outer loop calls policy.forward once per environment step (algorithm/sac.py:319-326), which reaches
 * Mamba.step (models/smamba/mamba.py:257-305; its GPU branch calls causal_conv1d_update and the Triton
 * selective_state_update, mamba_ssm/ops/triton/selective_state_update.py:21-154) and, for cgpt, flash-attn's MHA with
 * InferenceParams (models/flash_attention/TransformerFlashAttention.py:13-27,76-81; models/rnn_base.py:437-452).
 * All three read the old state and write a NEW state buffer (functional, like the reference's returned hidden), take
 * row strides in elements, and read nothing from the host - so a whole policy step can be captured in a hipGraph.
 *
 * resel_mamba_conv_step: window[b, d, :] <- (window[b, d, 1:], x[b, d]);  xc = act(sum_k taps * w[d, k] + bias[d]) over the
 *   newest K - 1 stored taps + x.  x [B, Di] (row stride ldx); state rows (strides ld_in / ld_out) hold W taps per channel at
 *   [d * stride_d + j * stride_k], oldest first: W = K, strides (K, 1) for smamba's [Di, K] window; W = K - 1, strides
 *   (1, Di) for the time-major [K - 1, Di] tail of the s6 `mamba` and `conv1d` layers (models/s6/mamba.py:166-176,
 *   models/conv1d/conv1d.py:27-37).  w [Di, K], bias [Di] or NULL; act: 1 = SiLU, 0 = none.
 * resel_selective_state_update: dt = softplus(x_db[:, :R] w_dt^T + dt_bias); A = -exp(A_log);
 *   h <- h * exp(dt A) + dt * Bm * xc;  y = sum_n h * Cm + D * xc;  y *= silu(z) if z.
 *   x_db [B, R + 2N] = (dt low-rank | Bm | Cm) (row stride ld_xdb), w_dt [Di, R], state [B, Di, N], z [B, Di] (row stride ldz).
 * resel_attn_decode: appends this token's k, v to kv_cache [Bmax, max_seqlen, 2, H, hd] (bf16) at position `pos` and
 *   returns softmax_j<=pos(scale q.k_j - slope_h (pos - j)) v_j as out [B, H, hd] bf16.  qkv [B, 3, H, hd] bf16 (row stride
 *   ld_qkv).  pos = *pos_dev when pos_dev != NULL (device step counter: graph replay), else pos_host.  hd in {32, 64, 128} (other widths: resel_head_pad).
 *   pos >= max_seqlen: RESEL_EINVAL for a host position; with a device counter the output row is NaN (the reference's
 *   flash-attn asserts on a full cache).
 * resel_attn_decode_rows: resel_attn_decode with ONE POSITION PER ROW - pos_rows [B] int32 on the device replaces pos_dev / pos_host.
 *   Row b appends its k, v at pos_rows[b] of its own cache slab and attends over keys 0..pos_rows[b] of that slab; its arithmetic
 *   depends on its own position only, so its output equals what resel_attn_decode gives for that row alone, bit for bit.  A row
 *   whose position is outside [0, max_seqlen) gets the NaN pattern in its own output rows and writes nothing else; the other rows
 *   are unaffected.  Rows of one graph replay may so be at different points of their episodes.
 * resel_step_state_reset: the start of an episode for SOME rows of a B-row step, as one kernel (one launch, nothing else on the
 *   stream, no allocation: capturable).  flags [B] int32 on the device, non-zero = row b starts an episode.  For every flagged row b:
 *   zeros over base[b * row_stride .. + width) of each of the nseg <= 16 segments (fp32; row_stride >= width, in elements - state
 *   tensors may be column views of wider rows; base 4-byte aligned) and 0 to pos[b] of each of the ncounters <= 8 int32 position
 *   arrays (the cgpt positions above).  Unflagged rows, and the gaps between the rows of a view, are not touched.  Both tables
 *   travel by value.  16-byte stores over the 16-byte aligned part of a row, 4-byte stores on its head and tail. */
#define RESEL_RESET_MAX_SEGS 16
#define RESEL_RESET_MAX_COUNTERS 8
typedef struct { float* base; int64_t row_stride; int32_t width; } resel_reset_seg_t;
typedef struct { resel_reset_seg_t seg[RESEL_RESET_MAX_SEGS]; } resel_reset_segs_t;
typedef struct { int32_t* pos[RESEL_RESET_MAX_COUNTERS]; } resel_reset_counters_t;
int resel_mamba_conv_step(const float* x, int64_t ldx, const float* state_in, int64_t ld_in, float* state_out, int64_t ld_out,
                          int64_t stride_d, int64_t stride_k, int W, const float* w, const float* bias, float* xc, int B, int Di,
                          int K, int act, resel_stream_t stream);
int resel_selective_state_update(const float* state_in, int64_t ld_in, float* state_out, int64_t ld_out, const float* xc,
                                 const float* x_db, int64_t ld_xdb, const float* w_dt, const float* dt_bias, const float* A_log,
                                 const float* D, const float* z, int64_t ldz, float* y, int B, int Di, int N, int R,
                                 resel_stream_t stream);
int resel_attn_decode(const uint16_t* qkv, int64_t ld_qkv, uint16_t* kv_cache, const int32_t* pos_dev, int pos_host,
                      const float* slopes, uint16_t* out, float scale, int B, int H, int head_dim, int max_seqlen,
                      resel_stream_t stream);
int resel_attn_decode_rows(const uint16_t* qkv, int64_t ld_qkv, uint16_t* kv_cache, const int32_t* pos_rows, const float* slopes,
                           uint16_t* out, float scale, int B, int H, int head_dim, int max_seqlen, resel_stream_t stream);
int resel_step_state_reset(const int32_t* flags, int B, resel_reset_segs_t segs, int nseg, resel_reset_counters_t counters,
                           int ncounters, resel_stream_t stream);

/* Categorical head of one policy step: policy_value_models/contextual_sac_discrete_policy.py:106-121 (softmax, probability floor,
 * renormalisation, torch.distributions.Categorical's own renormalisation, .mode, .sample(), log of all probabilities) as ONE launch
 * on `stream` - no LDS, no atomics, no allocation, nothing read from the host: capturable.  Per row of logits [M, A] (row stride
 * ld_logits):  s = softmax(x) (max-shifted, accurate expf);  t = s + floor;  p = t / sum(t);  p = p / sum(p);  logp = log(p).
 *   logp   [M, A] (row stride ld_logp);
 *   mode   [M]: the lowest index among the maxima of p;
 *   sample [M]: the smallest k with u[m] < p_0 + ... + p_k, clamped to A - 1; u [M] holds one uniform draw in [0, 1) per row and
 *               comes from the caller, as the noise of the tanh-Gaussian head does.
 * mode and sample are written as fp32 at mode[m * ld_idx] / sample[m * ld_idx], so that both may be columns of the row block that
 * also holds logp (the output block of a graphed step).  1 <= A <= RESEL_CATEGORICAL_MAX_ACTIONS, M >= 0 (M = 0: nothing is
 * launched, returns 0); anything else, a NULL pointer, ld_logits < A, ld_logp < A or ld_idx < 1: RESEL_EINVAL before the device
 * is touched.  A row that holds a NaN (or +inf) logit gets NaN in all of its logp, mode 0 and sample A - 1; the other rows are
 * unaffected and nothing asserts on the device. */
#define RESEL_CATEGORICAL_MAX_ACTIONS 4096
int resel_categorical_step(const float* logits, int64_t ld_logits, const float* u, float floor, float* logp, int64_t ld_logp,
                           float* mode, float* sample, int64_t ld_idx, int M, int A, resel_stream_t stream);

/* Environment step as the last node of a graphed policy step: the T-Maze memory task (reference envs/memory_envs/tmaze.py, TMazeBase
 * with ambiguous positions; ids and constants of envs/memory_envs/configs/tmaze_{passive,active}.py) for the B rows of a batched
 * evaluation - the per-row body of utility/policy_eval.py `run_episodes` and its `begin()`, as ONE launch on `stream`: one thread per
 * row, no LDS, no atomics, no allocation, nothing read from the host: capturable.
 *   cfg: cells (x, 0) for 0 <= x <= oracle_length + corridor_length and (oracle_length + corridor_length, +-1); an episode lasts
 *     episode_length steps; the three rewards are doubles and the reward of a step is formed in double exactly as the host
 *     environment forms it (env_utils/tmaze.py), signed zeros included.
 *   action: the fp32 action index of row b at action[b * ld_action] (column 0 of the categorical head's output block), clamped into
 *     [0, 4) (NaN: 0); 0..3 move by (1,0), (0,1), (-1,0), (0,-1), a move off the map leaves the position unchanged.
 *   goals [B, J] int32 (row stride ld_goals >= J): goal side -1 / +1 of the j-th episode of row b; n_episodes [B] int32: the episodes
 *     row b runs, clamped into [0, J].
 *   env_state [B, RESEL_TMAZE_STATE_WORDS] int32: x, y, goal_y, oracle_visited, t, ep_len, episodes_started, running;  ret_acc [B]
 *     double: the return of the running episode;  ep_ret double / ep_len int32 [B, J] (row stride ld_ep >= J): results per episode.
 *   in_block: the step's input rows (row stride ld_in >= 2 * 2 + A + 1): state[2] | lst_state[2] | lst_action[A] | reward[1];
 *     flags [B] int32: the step's reset flags.  Columns beyond the row's 2 * 2 + A + 1 are not touched.
 * init != 0: `begin()` for every row and no step: all state words written, lst_state = lst_action = reward = 0, flag = 1, ret_acc = 0;
 *   a row with n_episodes > 0 resets its environment with goals[b, 0] and gets the reset observation in `state`, any other row is
 *   idle with state = 0.  Every evaluation starts with this call; nothing is assumed about the buffers before it.
 * init == 0, idle row: zeros in the whole input row and flag = 1, nothing else.  Running row: the environment steps; lst_state <-
 *   state, state <- the new observation, lst_action <- one-hot(index), reward <- (float)r, ret_acc += r (double, in step order),
 *   ep_len += 1, flag = 0; when the episode is over ret_acc and ep_len go to [b, j], and the row begins episode j + 1 as above or
 *   goes idle once it has run n_episodes[b].
 * RESEL_EINVAL before the device is touched: a NULL pointer, A != 4, B < 0, J < 1, ld_in < 2 * 2 + A + 1, ld_action < 1, ld_goals < J,
 * ld_ep < J, corridor_length < 1, oracle_length < 0, episode_length < 1, penalty > 0.  B == 0 launches nothing and returns 0. */
#define RESEL_TMAZE_STATE_WORDS 8
typedef struct { int32_t corridor_length, oracle_length, episode_length; double goal_reward, penalty, distract_reward; } resel_tmaze_cfg_t;
int resel_tmaze_step(resel_tmaze_cfg_t cfg, int init, const float* action, int64_t ld_action, const int32_t* goals, int64_t ld_goals,
                     const int32_t* n_episodes, int J, int32_t* env_state, double* ret_acc, double* ep_ret, int32_t* ep_len,
                     int64_t ld_ep, float* in_block, int64_t ld_in, int A, int32_t* flags, int B, resel_stream_t stream);

/* ---- T-Maze training rollout inside the graphed policy step: one iteration of the collection loop per replay ----------------
 * (reference algorithm/sac.py:319-353: sample, env.step, mem_push of the transition, the next step's inputs; host twin: `SAC._train_loop`
 * with `SAC._push` / `SAC.env_step`, buffers/transition_buffer/replay_memory.py `transition_to_array`).  The LAST node of the policy step's
 * graph, as the entry above, with the same environment arithmetic (shared device functions) and the same env_state words; what differs is
 * that the action is the SAMPLED index (column 1 of the categorical step's block), that every step also writes the transition the ring
 * stores, and that a row never begins an episode by itself: the host starts each one with an init call outside the graph.
 *   action [B] fp32, stride ld_action: the sampled indices, clamped into [0, 4) (NaN: 0).   goal [B] int32: the goal side of the episode
 *     an init call begins (-1 / +1; read by init only).   env_state int32 [B, 8], ret_acc double [B]: word 5 is the number of steps taken,
 *     word 7 whether the episode runs; ret_acc the return so far, summed in double in step order.
 *   traj fp32 [B, T_cap, ld_row]: the episode block; step `len` (0-based) of row b writes transition row [b, len, :].
 *   lay: the first column of each ring field in a transition row (`MemoryArray.name2range`), -1 = the ring does not store it.  Widths:
 *     state, last_state, next_state 2; last_action A; action, reward, mask, start, done, reward_input, timeout 1.  The rollout has no
 *     log-probability: lay.logp must be -1.  Fields may stand in any order; columns no field covers are not touched.
 *   in_block fp32 [B, ld_in]: state[2] | lst_state[2] | lst_action[A] | reward[1], the policy step's input rows.
 * init != 0: `env_reset()` for every row and no step: state words zeroed, the environment reset with goal[b], ret_acc = 0, the reset
 *   observation in `state`, zeros in lst_state / lst_action / reward; the row runs.  traj is not touched.
 * init == 0, running row, step len: with `old` the input row as the policy step just read it and a the clamped index, the environment
 *   steps; traj[b, len] <- state, last_state, last_action, reward_input = old;  action = (float)a;  next_state = the new observation;
 *   reward = (float)r;  mask = 1;  start = (len == 0);  done;  timeout = (len + 1 >= max_episode_steps);  then the input row becomes
 *   lst_state <- old state, state <- the new observation, lst_action <- one-hot(a), reward <- (float)r;  ret_acc += r;  len += 1;  at
 *   done the row stops.  A step with len >= T_cap writes no transition row (everything else proceeds).
 * init == 0, stopped row: nothing is read or written.
 * RESEL_EINVAL before the device is touched: a NULL pointer, A != 4, B < 0, T_cap < 1, max_episode_steps < 1, ld_in < 2 * 2 + A + 1,
 * ld_action < 1, lay.logp >= 0, ld_row smaller than the furthest end of a present field, or a cfg the entry above refuses.  B == 0
 * launches nothing and returns 0.  One thread per row; no LDS, atomics, host read or allocation: capturable. */
typedef struct { int32_t state, last_state, last_action, action, next_state, reward, logp, mask, start, done, reward_input, timeout; } resel_collect_layout_t;
int resel_tmaze_collect_step(resel_tmaze_cfg_t cfg, resel_collect_layout_t lay, int init, const float* action, int64_t ld_action,
                             const int32_t* goal, int32_t* env_state, double* ret_acc, float* traj, int T_cap, int64_t ld_row,
                             int max_episode_steps, float* in_block, int64_t ld_in, int A, int B, resel_stream_t stream);

/* ---- Wind-v0 (reference envs/meta/toy_navigation/wind.py behind envs/meta/wrappers.py VariBadWrapper; host twin env_utils/wind.py):
 * the two entries above for a continuous-action environment.  Same shape - the LAST node of a graphed policy step, one thread per row,
 * 64-thread blocks, no LDS, no atomics, no allocation, nothing read from the host: capturable - and the same episode handling; what
 * differs is the state, the payload of an episode (its wind) and the action, which is the row's A = 2 fp32 values at
 * action[b * ld_action + 0 .. 1]: the Gaussian head's `mean` columns for the evaluation, its `sample` columns for the rollout.
 *   env_pos [B, RESEL_WIND_STATE_DOUBLES] double: x, y, wind_x, wind_y, and the position before the last step (last_x, last_y);
 *   env_words [B, RESEL_WIND_STATE_WORDS] int32: clock (steps of the episode), ep_len, episodes_started, running.
 *   in_block rows: state[2] | lst_state[2] | lst_action[2] | reward[1]  (ld_in >= 7).
 * A step is `env.step(unorm_act(a, env.action_space))` of the host loops, per component, every operation ONE correctly rounded
 * operation of the stated width, never contracted:
 *     t = (a + 1) / 2                                   in fp32 (the fp32 action meets Python scalars)
 *     u = (double)t * out_span + out_low                the outward Box(-1, 1) with double bounds
 *     c = clip(u, -1, 1);   v = act_low + ((c + 1.0) * 0.5) * act_span;   v = clip(v, act_low, act_high)
 *     p = (p + v) + wind                                the new position
 *   clock += 1;  done = clock >= episode_length;  dx = x - goal_x, dy = y - goal_y;  r = sqrt(dx * dx + dy * dy) <= goal_radius ? 1.0 : 0.0.
 *   clip(x, lo, hi) is numpy's: min(max(x, lo), hi) with a NaN passing through.  So a NaN action component makes that component of
 *   the position NaN for the rest of the episode: the observation carries the NaN, the reward is 0.0, the clock and `done` are unaffected.
 *   cfg carries the bounds as the doubles the host arithmetic meets: act_low / act_high the fp32 +-0.1 promoted, act_span their fp32
 *   difference promoted, out_low and out_span = high - low of the outward box.
 * The next input row: lst_state <- state, state <- (float)position, lst_action <- a as read (bits kept), reward <- (float)r.
 * evaluation entry: winds [B, J, 2] double (row stride ld_winds >= 2 J doubles): the wind of the j-th episode of row b; n_episodes, ret_acc,
 *   ep_ret, ep_len, flags, init, idle rows and the hand-over at an episode's end as in the T-Maze evaluation entry (a reset puts the
 *   position at (0, 0), last position (0, 0), and the episode's wind into env_pos).
 * rollout entry: wind [B, 2] double, read by init only; traj, lay, T_cap, ld_row, max_episode_steps, init, stopped rows as in the
 *   T-Maze rollout entry, except that the `action` field of a transition row is A columns wide and holds a as read.
 * RESEL_EINVAL before the device is touched: a NULL pointer, A != 2, B < 0, ld_in < 7, ld_action < 2, episode_length < 1, a goal_radius
 *   that is not >= 0, act_low > act_high, a NaN in cfg; evaluation: J < 1, ld_winds < 2 J, ld_ep < J; rollout: T_cap < 1,
 *   max_episode_steps < 1, lay.logp >= 0, ld_row smaller than the furthest end of a present field.  B == 0 launches nothing, returns 0. */
#define RESEL_WIND_STATE_DOUBLES 6
#define RESEL_WIND_STATE_WORDS 4
typedef struct { int32_t episode_length; double goal_x, goal_y, goal_radius, act_low, act_high, act_span, out_low, out_span; } resel_wind_cfg_t;
int resel_wind_step(resel_wind_cfg_t cfg, int init, const float* action, int64_t ld_action, const double* winds, int64_t ld_winds,
                    const int32_t* n_episodes, int J, double* env_pos, int32_t* env_words, double* ret_acc, double* ep_ret, int32_t* ep_len,
                    int64_t ld_ep, float* in_block, int64_t ld_in, int A, int32_t* flags, int B, resel_stream_t stream);
int resel_wind_collect_step(resel_wind_cfg_t cfg, resel_collect_layout_t lay, int init, const float* action, int64_t ld_action,
                            const double* wind, double* env_pos, int32_t* env_words, double* ret_acc, float* traj, int T_cap, int64_t ld_row,
                            int max_episode_steps, float* in_block, int64_t ld_in, int A, int B, resel_stream_t stream);

/* ---- Catch-<runs>-v0 (reference envs/credit_assign/catch.py DelayedCatch; host twin env_utils/catch.py): the T-Maze pair of entries
 * for the delayed-reward task.  Same shape - the LAST node of a graphed policy step, one thread per row, 64-thread blocks, no LDS, no
 * atomics, no allocation, nothing read from the host: capturable - and the same episode handling; what differs is the state, the
 * payload of an episode (a table of draws) and the widths: A = 3 actions, a 49-wide observation.
 *   cfg: num_catches runs of 7 steps (6 falling steps, then - except behind the last run - one soft-reset step);
 *     episode_length = 7 * num_catches - 1.
 *   action: the fp32 action index of row b at action[b * ld_action] (evaluation: column 0 of the categorical head's output block, the
 *     mode; rollout: column 1, the sample), clamped into [0, 3) (NaN: 0); 0 / 1 / 2 move the basket left / not / right.
 *   draws: one episode's payload is 2 * RESEL_CATCH_MAX_RUNS int32, the fruit columns ns[40] first, then the basket start columns
 *     ms[40]; entries behind num_catches are not read by a step (the host sends zeros).  Evaluation: draws [B, J, 80] with row stride
 *     ld_draws >= 80 J; rollout: draws [B, 80], read by init only.
 *   env_state [B, RESEL_CATCH_STATE_WORDS] int32: fruit_row, fruit_col, basket, catch_count, t, accumulated, ep_len, episodes_started,
 *     running, a pad word, ns[40], ms[40] - a reset copies the episode's draws into the row, a step never reads the payload.
 *   in_block rows: state[49] | lst_state[49] | lst_action[3] | reward[1]  (ld_in >= 102).  The observation is the flattened 7 x 7
 *     canvas: -1 at (fruit_row, fruit_col), then +1 at (6, basket), everything else 0; a caught fruit is covered by the basket.
 * A step: t += 1.  fruit_row == 6 (the steps t = 7 k): the action is ignored, (fruit_row, fruit_col, basket) <- (0, ns[c], ms[c]) with
 *   c = catch_count clamped into [0, num_catches), catch_count <- c + 1, reward 0, not done.  Otherwise basket <- clip(basket + a - 1,
 *   0, 6), fruit_row += 1, accumulated += 1 when fruit_row == 6 and fruit_col == basket; done = t >= episode_length; the reward is
 *   (double)accumulated on the done step and 0.0 before it.  Rows, columns and the count are clamped where they index: a corrupted
 *   state word never becomes an access outside the row.
 * The next input row: lst_state <- state, state <- the new observation, lst_action <- one-hot(a), reward <- (float)r.
 * n_episodes, ret_acc, ep_ret, ep_len, flags, init, idle rows and the hand-over at an episode's end as in the T-Maze evaluation entry;
 * traj, lay (widths: state, last_state, next_state 49; last_action 3; everything else 1; lay.logp = -1), T_cap, ld_row,
 * max_episode_steps, init and stopped rows as in the T-Maze rollout entry.
 * RESEL_EINVAL before the device is touched: a NULL pointer, A != 3, B < 0, ld_in < 102, ld_action < 1, num_catches < 1 or >
 *   RESEL_CATCH_MAX_RUNS, episode_length != 7 * num_catches - 1; evaluation: J < 1, ld_draws < 80 J, ld_ep < J; rollout: T_cap < 1,
 *   max_episode_steps < 1, lay.logp >= 0, ld_row smaller than the furthest end of a present field.  B == 0 launches nothing, returns 0. */
#define RESEL_CATCH_MAX_RUNS 40
#define RESEL_CATCH_STATE_WORDS 90
typedef struct { int32_t num_catches, episode_length; } resel_catch_cfg_t;
int resel_catch_step(resel_catch_cfg_t cfg, int init, const float* action, int64_t ld_action, const int32_t* draws, int64_t ld_draws,
                     const int32_t* n_episodes, int J, int32_t* env_state, double* ret_acc, double* ep_ret, int32_t* ep_len,
                     int64_t ld_ep, float* in_block, int64_t ld_in, int A, int32_t* flags, int B, resel_stream_t stream);
int resel_catch_collect_step(resel_catch_cfg_t cfg, resel_collect_layout_t lay, int init, const float* action, int64_t ld_action,
                             const int32_t* draws, int32_t* env_state, double* ret_acc, float* traj, int T_cap, int64_t ld_row,
                             int max_episode_steps, float* in_block, int64_t ld_in, int A, int B, resel_stream_t stream);

/* ---- discrete-action update: differentiable categorical head, all-action value, the two discrete losses --------------------
 * (reference contextual_sac_discrete_policy.py:106-121 on whole rows; sac_full_length_rnn_redq.py:52-72 target, :85-86 actor,
 * sac_full_length_rnn_ensembleQ.py:158 critic on the action taken).  Raw fp32 device pointers; logits / logp / probs [M, A];
 * q / dq [E, M, A] contiguous, A fastest; mask / y / v / action [M]; g and log_alpha device scalars.  Every entry returns
 * RESEL_EINVAL before the device is touched for a NULL required pointer, A < 1, A > RESEL_CATEGORICAL_MAX_ACTIONS, E < 1 or M < 0;
 * M == 0 launches nothing and returns 0.  No host read, no device assert, no atomics (sums are two-stage in a fixed order: bitwise
 * reproducible), capturable.
 *
 * head, forward: the four steps of resel_categorical_step (one shared device function) on every row: logp = log p, probs = p,
 *   mode [M] = the lowest argmax of p as fp32; no sampling.  A row holding a NaN gets NaN in all of its logp and probs and mode 0;
 *   other rows are unaffected.  A row takes the next power of two at or above A lanes (at most 64), a wave 64 / that rows; A > 64
 *   runs the chunked loop of the step kernel.
 * head, backward: dlogp or dprobs may be NULL (both NULL: RESEL_EINVAL).  With s = softmax(x), S2 = sum(s + floor), p the final
 *   probabilities:  g_i = dprobs_i + dlogp_i / p_i;  dp_i = g_i - sum_j g_j p_j;  ds_i = dp_i / S2;  dx_i = s_i (ds_i - sum_j ds_j s_j).
 *   s and p are recomputed from the logits, so the call takes the same `floor` as the forward.  A = 1: dlogits is exactly 0. */
int resel_categorical_fwd(const float* logits, float floor, float* logp, float* probs, float* mode, int M, int A, resel_stream_t stream);
int resel_categorical_bwd(const float* logits, float floor, const float* dlogp, const float* dprobs, float* dlogits, int M, int A,
                          resel_stream_t stream);
/* all-action value (no gradient):  v[r] = sum_a exp(logp[r, a]) (min_{e in S} q[e, r, a] - exp(log_alpha) logp[r, a]);  S = the m
 * entries of subset (int32, device; clamped into [0, E)) or, subset == NULL, all E members (m is ignored).  A NaN member gives NaN. */
int resel_discrete_value(const float* q, const int32_t* subset, int m, const float* logp, const float* log_alpha, float* v,
                         int E, int M, int A, resel_stream_t stream);
/* critic loss on the action taken: action [M] is the fp32 index as the batch stores it, clamped into [0, A) before the read (NaN: 0).
 *   out2[0] = sum_m mask sum_e (q[e, m, a_m] - y[m])^2                                  (mask NULL = ones)
 *   dq[e, m, a] = 2 g[0] mask (q[e, m, a_m] - y[m]) at a = a_m, 0 elsewhere; EVERY element of dq is written; rows with mask == 0 get 0.
 * workspace: resel_masked_loss_workspace_bytes(). */
int resel_q_taken_loss_fwd(const float* q, const float* action, const float* y, const float* mask, float* out2, void* workspace,
                           int E, int M, int A, resel_stream_t stream);
int resel_q_taken_loss_bwd(const float* q, const float* action, const float* y, const float* mask, const float* g, float* dq,
                           int E, int M, int A, resel_stream_t stream);
/* actor loss as an expectation over all actions: p = exp(logp), alpha = exp(log_alpha), Q_a = min_e (reduce_min 1) or mean_e (0) q[e, ., a]
 *   out2[0] = sum_m mask sum_a p_a (alpha logp_a - Q_a),   out2[1] = sum_m mask sum_a p_a logp_a   (a statistic: no gradient)
 *   dlogp[m, a] = g[0] mask p_a (alpha (logp_a + 1) - Q_a)
 *   dq (may be NULL: not formed) = -g[0] mask p_a / E (mean)  or  -g[0] mask p_a at the FIRST minimal member, 0 elsewhere (min). */
int resel_discrete_actor_loss_fwd(const float* logp, const float* q, const float* mask, const float* log_alpha, float* out2,
                                  void* workspace, int E, int M, int A, int reduce_min, resel_stream_t stream);
int resel_discrete_actor_loss_bwd(const float* logp, const float* q, const float* mask, const float* log_alpha, const float* g,
                                  float* dlogp, float* dq, int E, int M, int A, int reduce_min, resel_stream_t stream);

/* ---- C = W^T N over a very long reduction dimension (weight gradients of the narrow Mamba projections) ----------------
 * Replaces autograd's `grad.t() @ input` of the x_proj / dt_proj F.linear calls (reference
 * models/smamba/mamba_ssm/ops/selective_scan_interface_new.py:261-335; models/smamba/mamba.py:231-233).
 * wide [K, Wd] (row stride ldw, Wd % 4 == 0, 16-byte aligned rows), narrow [K, Nd <= 96] (row stride ldn);
 * out = wide^T narrow as [Wd, Nd], or its transpose [Nd, Wd] when transposed != 0.  fp32 MFMA, the reduction is split over
 * the grid and summed in a fixed order (deterministic).  workspace: resel_atb_workspace_bytes(K, Wd, Nd). */
size_t resel_atb_workspace_bytes(int64_t K, int Wd, int Nd);
int resel_atb(const float* wide, int64_t ldw, int Wd, const float* narrow, int64_t ldn, int Nd, float* out, int transposed,
              void* workspace, int64_t K, resel_stream_t stream);

/* Products with one side at most 48 wide, bound by one pass over their wide side (csrc/skinny_gemm.hip; fp32 MFMA, no operand split).
 *
 * resel_narrow_k: C[M, N] (row stride ldc) = act(A[M, :K] W[N, K]^T + bias[N]).  K <= 48, K % 4 == 0, N % 4 == 0; A is a column block
 * of a wider row-major matrix (row stride lda, 8-byte aligned, lda even); W has row stride ldw (8-byte aligned, even); C is 16-byte
 * aligned with ldc % 4 == 0.  act: 0 none, 1 ELU, 3 softplus (the codes of resel_gemm_f32x).  bias may be NULL.  amax_out: magnitude
 * handle that receives max |C| under amax_epoch, or NULL.  One launch, no workspace.
 *
 * resel_narrow_n_pair: one pass over G[M, Wd] (row stride ldg % 4 == 0, 16-byte aligned, Wd % 4 == 0, Wd <= 512) gives
 *   dX[M, Nn] (row stride lddx) = G W[Wd, Nn] (row stride ldw)      and      dW[Wd, Nn] (dense) = G^T X[M, Nn] (row stride ldx),
 * Nn <= 48.  Either output may be NULL (then its second operand is not read).  dX is summed over Wd inside the workgroup, dW over M
 * as resel_atb does (partial slabs in `workspace`, resel_narrow_n_pair_workspace_bytes(M, Wd, Nn), added in a fixed order): both are
 * bitwise reproducible.  Shapes outside these limits return RESEL_EINVAL; callers keep the GEMM route for them. */
int resel_narrow_k(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, float* C, int64_t ldc, int64_t M, int N,
                   int K, int act, void* amax_out, unsigned amax_epoch, resel_stream_t stream);
size_t resel_narrow_n_pair_workspace_bytes(int64_t M, int Wd, int Nn);
int resel_narrow_n_pair(const float* G, int64_t ldg, int Wd, const float* W, int64_t ldw, const float* X, int64_t ldx, int Nn, float* dX,
                        int64_t lddx, float* dW, void* workspace, int64_t M, resel_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RESEL_HIP_H */
