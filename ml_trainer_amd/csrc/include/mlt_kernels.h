// Host-visible launcher interface of the gfx950 kernels (csrc/kernels/*.hip).
// Pure HIP types only: the torch glue lives in csrc/bindings.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlt_optim.h"
#include "mlt_philox.h"

namespace mlt {

// ----------------------------------------------------------------------------
// Flat optimizers (optim.hip)
// ----------------------------------------------------------------------------
// lr = lr_ptr ? lr_ptr[lr_index_ptr ? (*lr_index_ptr - 1) : 0] : h.lr
// t  = step_ptr ? *step_ptr : t_host           (1-based step count)
void launch_flat_optim(float* p, const float* g, float* s1, float* s2, int64_t n, const OptHyper& h,
                       const float* lr_ptr, const int64_t* lr_index_ptr, const int64_t* step_ptr, float t_host,
                       uint16_t* shadow_bf16, const float* coef_ptr, hipStream_t stream,
                       const unsigned* skip = nullptr);  // skip: no update while *skip != 0
// Per-tensor updates through a segment table over the flat buffer (built by ops/optim.py):
//   chunks[nchunks][4] = {tensor id, first float4, float4 count (<= optim_chunk_elems() / 4), 0}
//   tseg[nt][2] = {first chunk, chunk count}; wd[nt]; adapt[nt] (0/1)
// lr / step / coef / skip as launch_flat_optim. max_blocks > 0 lowers the block cap (results do not
// depend on it). An entry that points outside the buffer or the tables is skipped by the kernels.
int optim_chunk_elems();
// AdamW with weight_decay = wd[tensor], one launch; a tensor's bits equal launch_flat_optim's with that decay
void launch_flat_optim_seg(float* p, const float* g, float* s1, float* s2, int64_t n, const int* chunks,
                           int nchunks, const float* wd, int nt, const OptHyper& h, const float* lr_ptr,
                           const int64_t* lr_index_ptr, const int64_t* step_ptr, float t_host,
                           uint16_t* shadow_bf16, const float* coef_ptr, const unsigned* skip, int max_blocks,
                           hipStream_t stream);
// LAMB: stage 1 (moments, per-chunk sums of w^2 and u^2 -> part[nchunks][2]), finalize (norms[nt][2] = the sums
// of squares, trust[nt]), stage 2 (apply, shadow). stages: bit 0 / 1 / 2 selects the launches (7 = a step).
void launch_lamb_step(float* p, const float* g, float* m, float* v, int64_t n, const int* chunks, int nchunks,
                      const int* tseg, const float* wd, const int* adapt, int nt, float* part, float* norms,
                      float* trust, const OptHyper& h, const float* lr_ptr, const int64_t* lr_index_ptr,
                      const int64_t* step_ptr, float t_host, uint16_t* shadow_bf16, const float* coef_ptr,
                      const unsigned* skip, int max_blocks, int stages, hipStream_t stream);
// out[0] = sum of squares of x[0..n): per-block partials into `part` (sq_norm_partials_needed() floats,
// contents irrelevant), then summed in block order -> bitwise reproducible. out is overwritten.
int sq_norm_partials_needed();
void launch_sq_norm(const float* x, int64_t n, float* part, float* out, hipStream_t stream);
void launch_clip_coef(const float* sq, float max_norm, float* coef, float* total_norm, hipStream_t stream);
void launch_cast_bf16(const float* x, uint16_t* y, int64_t n, hipStream_t stream);
// dst[C][R] = src[R][C], bf16 (transpose.hip)
void launch_transpose_bf16(const uint16_t* src, uint16_t* dst, int R, int C, hipStream_t stream);

// ----------------------------------------------------------------------------
// LeNet-5 (reference src/model.py:7-24) fused forward/backward (lenet.hip)
// ----------------------------------------------------------------------------
enum LeNetCfg : int { LENET_DEFAULT = 0, LENET_TINY = 1 };
enum LeNetMode : int {
  LENET_FWD = 1,        // conv1 -> logits
  LENET_CE = 2,         // softmax-CE loss + dlogits + loss/accuracy accumulation
  LENET_BWD = 4,        // dlogits -> all parameter gradients
  LENET_OPT = 8,        // fused optimizer update inside the weight-gradient kernel (single process only)
  LENET_REDUCE = 16,    // data-parallel step (LeNetEngine): all-reduce the flat gradient after the backward
                        // kernels, then the flat optimizer update; exclusive with LENET_OPT
  LENET_TRACE = 256,    // bf16 kernels only (MLT_LENET_TRACE_BUILD): phase stamps into LeNetPtrs::trace
  LENET_STATS_DEFER = 16384,  // internal: CE writes per-sample loss / hit to cestat; K4 sums them in sample order
  // timing probes of the bf16 per-sample kernel (wrong numerics: profiling only; env MLT_LENET_PROBE)
  LENET_PROBE_NOF1T = 1 << 17,  // role A skips the fc1 dgrad (transposed) weight fetch
  LENET_PROBE_NOF1W = 1 << 18,  // role B skips the fc1 forward weight fetch
  LENET_PROBE_NOF2 = 1 << 19,   // fc2 forward + dgrad weight fetches skipped
  LENET_NOSPLIT = 1 << 20,      // internal: the bf16 per-sample kernel runs one block per sample (engine switch off)
  // internal: role-D parts per sample of the split per-sample kernel, 3 bits (0: auto, else that ND)
  LENET_SPLITD_SHIFT = 21,
  LENET_SPLITD_MASK = 7 << 21,
};

struct LeNetPtrs {
  const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4, *w5, *b5;  // params (fp32)
  float *gw1, *gb1, *gw2, *gb2, *gw3, *gb3, *gw4, *gb4, *gw5, *gb5;  // grads (fp32)
  float *x, *p1, *p2, *h1, *h2, *logits, *dlogits, *dh2, *dh1, *dflat, *g1, *slab1;
  uint8_t *i1, *i2;
  int64_t* targets;          // [B] class ids (written by conv1 in the augment path)
  const int64_t* dtargets;   // dataset targets [N] (augment path)
  double* stats;             // [2]: sum over batches of batch-mean loss, of batch accuracy
  unsigned* counters;        // [>= C1+1] zero-initialised; only [C1] is used: K5's launch-wide arrival counter
  uint8_t* stage;            // [B][3072] raw uint8 images of the next step (nullptr: no staging)
  int64_t* stage_meta;       // [B][4] (perm position, dataset row, target, 0) of each staged image; -1 = empty
  double* cestat;            // [B][2] per-sample (loss / B, hit / B) for the fixed-order stats sum (or nullptr)
  // bf16 MFMA engine (lenet_mfma.hip)
  uint8_t* stage2;           // [B][3072] raw uint8 images of the next step (staged by the per-sample kernel)
  int64_t* meta2;            // [B][4] (global step, perm position, dataset row, target) of each; -1 = empty
  int64_t* metaN;            // [B][4] (global step, perm position, perm entry, 0): lookup one step further
  int64_t* stepinfo;         // [4] (step, step in epoch, lr bits) of the running step, for the wgrad kernel
  uint16_t* shadow;          // bf16 copy of the flat fp32 parameters (fc weights are read from it)
  uint16_t* wimg;            // bf16 conv-weight MFMA fragment image (lenet_mfma_wimg_elems())
  float* trace;              // LENET_TRACE phase stamps (8-byte slots) or nullptr
  // next-step inputs prepared by the batch-reduction kernel's prep blocks (nullptr: off): the
  // augmented bf16 pixels [B][1024] x (c0, c1 | c2, 0) of the sample each block will compute next,
  // tagged pmeta[B][4] = (global step, perm position, target, 0); -1 = empty
  uint8_t* prep;
  int64_t* pmeta;
};

struct LeNetAug {
  const uint8_t* data;  // [N,32,32,3] HWC uint8; nullptr -> ptrs.x is the (normalised) input
  int64_t step_host, sie_host;  // used instead of ctrl[0], ctrl[1] when ctrl == nullptr
  const int32_t* perm;  // epoch sample order
  int64_t* ctrl;        // ctrl[0]: global step (1-based after the step), ctrl[1]: step in epoch
  int64_t n;            // dataset rows
  int64_t perm_len;
  uint64_t seed;
  int pad;              // RandomCrop padding (0 = no crop)
  int flip;             // RandomHorizontalFlip(p=0.5)
  int batch_stride;     // samples per step (offset into perm = ctrl[1]*batch_stride)
  float mean[3], std[3];
  float ascale[3], ashift[3];  // normalisation as one fma (bf16 engine): u * ascale + ashift
};

struct LeNetOpt {
  float *p, *g, *s1, *s2;  // whole flat buffers (params / grads / state)
  int64_t n;
  OptHyper h;
  const float* lr_ptr;     // device lr (table indexed by ctrl[1]-1 when lr_table)
  int lr_table;
  // flat-buffer offsets of the 10 LeNet tensors (w1,b1,w2,b2,w3,b3,w4,b4,w5,b5)
  int64_t off[10];
};

void launch_lenet(int cfg, int mode, int B, const LeNetPtrs& P, const LeNetAug& A, const LeNetOpt& O,
                  hipStream_t stream);
// BERT classifier head (head.hip): classifier layer of num_labels outputs on the VALU
void launch_head_cls_fwd(const float* pooled, int B, int h, const float* wc, const float* bc, int L, float* logits,
                         hipStream_t st);
void launch_head_cls_bwd(const float* dlogits, const float* pooled, const float* wc, int B, int h, int L,
                         uint16_t* dpre, float* dwc, float* dbc, bool accumulate, hipStream_t st);
// bf16 MFMA training step (lenet_mfma.hip): 2 launches per step (per-sample chain + batch
// reductions / optimizer). Needs stage2 / meta2 / stepinfo / shadow, and slab1 >= B * slab floats.
void launch_lenet_mfma(int cfg, int mode, int B, const LeNetPtrs& P, const LeNetAug& A, const LeNetOpt& O,
                       hipStream_t stream);
// whether that step's per-sample kernel would run two blocks per sample at batch B (split tail)
bool lenet_mfma_split_active(int mode, int B, const LeNetPtrs& P, const LeNetAug& A);
// blocks per sample of that launch: 1 unsplit, else ND + 1 (ND role-D parts sharing the conv1 wgrad
// by kernel column, and the role-W block); whether n is a LENET_SPLITD value the build carries
int lenet_mfma_split_blocks(int mode, int B, const LeNetPtrs& P, const LeNetAug& A);
bool lenet_mfma_split_parts_valid(int n);
int lenet_mfma_slab_floats(int cfg);
int lenet_mfma_kw_blocks(int cfg);  // grid of the batch-reduction / optimizer kernel
// data-parallel bf16 step: optimizer update from the all-reduced gradient + bf16 shadow + fragment
// images in one launch (skip: nonzero vetoes the update)
void launch_lenet_mfma_apply(int cfg, const LeNetPtrs& P, const LeNetOpt& O, const unsigned* skip, hipStream_t stream);
// data-parallel bf16 step in TWO launches (as at W = 1): the per-sample kernel, then the batch
// reductions + xGMI exchange + rank-ordered sum + update of every gradient element in one launch
// (struct XgmiFused; throws if X.G < lenet_mfma_kw_blocks(cfg) or X.W outside 1..8)
struct XgmiFused;
void launch_lenet_mfma_dp(int cfg, int mode, int B, const LeNetPtrs& P, const LeNetAug& A, const LeNetOpt& O,
                          const XgmiFused& X, hipStream_t stream);
int lenet_mfma_wimg_elems();
bool lenet_mfma_trace_build();  // LENET_TRACE stamps compiled in (MLT_LENET_TRACE_BUILD)
// batch reductions (+ the exchange when X) into O.g only, no update (transport self-test / timing)
void launch_lenet_mfma_reduce(int cfg, int B, const LeNetPtrs& P, const LeNetOpt& O, const XgmiFused* X,
                              hipStream_t stream);
int64_t lenet_mfma_xch_granules(int cfg);  // granules per parity the fused exchange needs
// shadow + wimg from the fp32 masters (O.p)
void launch_lenet_mfma_pack(int cfg, const LeNetPtrs& P, const LeNetOpt& O, hipStream_t stream);

// Standalone GPU augmentation (RandomCrop(32,pad) + HFlip + ToTensor + Normalize) for the
// generic (non-LeNet) device data path: out [B,3,32,32] fp32.
void launch_cifar_augment(const LeNetAug& A, int B, float* out, int64_t* targets_out, const int64_t* dtargets,
                          hipStream_t stream);

// ----------------------------------------------------------------------------
// Losses / metrics (losses.hip)
// ----------------------------------------------------------------------------
// acc[2] (zeroed by caller): {sum of row losses, number of valid rows}; loss[0] = mean.
void launch_ce_fwd(const void* logits, bool bf16, const int64_t* tgt, int64_t B, int C, float* dl, float* acc,
                   float* correct, float* loss, int64_t ignore_index, float label_smoothing, hipStream_t st);
void launch_ce_bwd(const float* dl, const float* gout, const float* acc, int64_t n, void* out, bool bf16,
                   hipStream_t st);
void launch_accuracy(const void* logits, bool bf16, const int64_t* tgt, int64_t B, int C, float* out,
                     hipStream_t st);
// Regression / NLL criteria and mcrmse (fp32). `part` holds loss_partials_needed() floats;
// out/stats[2] = {mean loss, denominator}; g is the unscaled elementwise gradient.
int loss_partials_needed();
void launch_pointwise_loss_fwd(const float* p, const float* t, int64_t n, int mode, float* g, float* part,
                               float* out, hipStream_t st);
void launch_nll_fwd(const float* logp, const int64_t* tgt, int64_t B, int C, int64_t ignore_index, float* part,
                    float* out, hipStream_t st);
void launch_loss_scale_grad(const float* g, const float* gout, const float* stats, int64_t n, float* out,
                            hipStream_t st);
void launch_nll_bwd(const int64_t* tgt, int64_t B, int C, int64_t ignore_index, const float* gout,
                    const float* stats, float* out, hipStream_t st);
void launch_mcrmse(const float* p, const float* t, int64_t B, int C, float* col, float* out, hipStream_t st);

// ----------------------------------------------------------------------------
// bf16 MFMA GEMM (gemm.hip): C[M,N] = alpha * op(A) . op(B) (+bias) (+epilogue)
//   a_mn: A stored [K][M] (else [M][K]);  b_mn: B stored [K][N] (else [N][K])
//   mode: 0 none, 1 GELU (pre-activation written to aux), 2 dGELU (multiply by gelu'(aux))
// ----------------------------------------------------------------------------
// Kernel choice per shape: cfg 0 = 128x128 register-staged kernel (any K % 8 == 0), cfg 1..4 =
// 256x256 / 256x128 / 128x256 / 256x192 global_load_lds kernels (K % 64 == 0) with split-K
// (deterministic in-launch slab reduction; needs ws_floats of fp32 workspace from the caller;
// tile counters come from an internal self-resetting pool when cnt == nullptr), cfg 5 = 256x256
// ping-pong kernel, cfg 7 = 4-wave asm kernel (gemm_w4.hip). cfg 6 (a persistent ping-pong kernel)
// is retired: the number stays unused and the bindings reject it.
struct GemmPlan {
  int cfg;
  int splits;
  int ksteps;  // K-steps (of 64) per split
  int64_t ws_floats;
  int64_t cnt_ints;
  int ext = 0;  // split-K partials summed by a separate grid-wide reduce launch (else: last-arriver in-kernel)
};
GemmPlan plan_gemm_bf16(int a_mn, int b_mn, int M, int N, int K, int force_cfg, int force_splits,
                        int accumulate = 0);
void set_gemm_split_mode(int mode);  // -1 planner, 0 in-kernel last-arriver, 1 external reduce
void set_gemm_w4q8(int on);          // gemm_f8_q GELU: 1 4-wave kernel, 0 ping-pong, -1 default (1)
void launch_gemm_bf16(const GemmPlan& plan, int a_mn, int b_mn, bool out_f32, const uint16_t* A, const uint16_t* B,
                      void* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, const float* bias,
                      const uint16_t* aux, int64_t ldaux, const uint16_t* res, int64_t ldres, float alpha, int mode,
                      int accumulate, float* ws, unsigned* cnt, hipStream_t st, float* colpart = nullptr);
// Weight-streaming GEMM for decode steps (gemm_skinny.hip): Y [M][N] = epilogue(X [M][K] . W [N][K]^T), both
// operands k-contiguous bf16 with 16-byte aligned rows, 1 <= M <= kSkinnyMaxRows, N % 16 == 0, K % 32 == 0; bias
// fp32 [N], mode 0 or 1 (GELU, writes the bf16 pre-activation to aux), res bf16 [M][N]. The summation order is a
// function of (N, K) alone: a row's result does not depend on M. No workspace, nothing allocated.
constexpr int kSkinnyMaxRows = 64;
void launch_gemm_skinny(const uint16_t* X, const uint16_t* W, void* Y, bool out_f32, int M, int N, int K, int64_t ldx,
                        int64_t ldw, int64_t ldy, const float* bias, const uint16_t* aux, int64_t ldaux,
                        const uint16_t* res, int64_t ldres, int mode, hipStream_t st);
// fp8 GEMM (gemm_tile.hip): A [M][K], B [N][K] both k-contiguous fp8 (fmt 0 = e4m3, 1 = e5m2),
// K % 128 == 0; alpha *= inv_scale_a[0] * inv_scale_b[0] (device scalars, delayed scaling).
GemmPlan plan_gemm_f8(int M, int N, int K, int force_cfg, int force_splits);
void launch_gemm_f8(const GemmPlan& plan, int fmt_a, int fmt_b, bool out_f32, const uint8_t* A, const uint8_t* B,
                    void* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, const float* inv_scale_a,
                    const float* inv_scale_b, const float* bias, const uint16_t* aux, int64_t ldaux,
                    const uint16_t* res, int64_t ldres, float alpha, int mode, int accumulate, float* ws,
                    unsigned* cnt, hipStream_t st);
// fp8 GEMM with a quantising epilogue (gemm_pp_kernel, OutT = uint8_t): Y = fp8(act(A.B^T*ia*ib
// + bias) * out_scale) [M,N] and Y^T [N,M] (mode 0 none, 1 GELU writing the bf16 pre-activation
// to aux, 2 dGELU reading it), amax of act(..) into out_amax, optional [M/64, N] column partials.
// M % 256 == 0, N % 256 == 0, K % 128 == 0; fmt_a e4m3 or e5m2, fmt_b e4m3.
void launch_gemm_f8_q(int fmt_a, int fmt_b, const uint8_t* A, const uint8_t* B, uint8_t* Y, uint8_t* Yt, int M, int N,
                      int K, int64_t lda, int64_t ldb, int64_t ldy, int64_t ldyt, const float* inv_scale_a,
                      const float* inv_scale_b, const float* bias, const uint16_t* aux, int64_t ldaux, int mode,
                      int out_fmt, const float* out_scale, float* out_amax, float* colpart, hipStream_t st);
// fp8 quantisation (fp8.hip); every amax argument points at kAmaxSlots slots spaced
// kAmaxStride floats apart (kAmaxSlots * kAmaxStride floats per tensor)
constexpr int kAmaxSlots = 64, kAmaxStride = 32;
void launch_cast_fp8(const void* x, bool x_f32, uint8_t* y, int64_t n, const float* scale, float* amax, int fmt,
                     hipStream_t st);
void launch_amax(const void* x, bool x_f32, int64_t n, float* amax, hipStream_t st);
void launch_cast_transpose_fp8(const float* w, uint8_t* y, uint8_t* yt, int R, int C, const float* scale, float* amax,
                               int fmt, hipStream_t st);
bool cast_transpose_fp8_wide_ok(const void* x, const void* y, const void* yt, int R, int C);
void launch_cast_transpose_fp8_bf16(const uint16_t* x, uint8_t* y, uint8_t* yt, int R, int C, const float* scale,
                                    float* amax, int fmt, hipStream_t st, float* colpart = nullptr);
void launch_fp8_update_scale(float* hist, int H, int n, float* amax, float* scale, float* inv_scale, const float* fmax,
                             int margin, int64_t step, hipStream_t st);

// one-shot xGMI all-reduce (allreduce.hip): peer region pointers indexed by rank
constexpr int kXgmiMaxRanks = 8;
struct XgmiPeers {
  float* data[kXgmiMaxRanks];
  uint64_t* flags[kXgmiMaxRanks];
  // two-shot (reduce-scatter + all-gather by remote pushes): per-rank [2][W][slot] staging of the
  // scattered slices (t1) and of the reduced slices (t2), each with its own [2][G][W] flags
  float* t1[kXgmiMaxRanks];
  float* t2[kXgmiMaxRanks];
  uint64_t* f1[kXgmiMaxRanks];
  uint64_t* f2[kXgmiMaxRanks];
};
// optional fused flat-optimizer update of the reduced slice (same semantics as
// launch_flat_optim with lr / step from device memory)
struct XgmiPostOpt {
  float *p, *s1, *s2;
  OptHyper h;
  const float* lr_ptr;
  const int64_t* lr_index_ptr;
  const int64_t* step_ptr;
};
// fault (tests only): 1 = this rank never publishes the slices b with b % (2 W) == rank, so on every
// rank those slices time out while the others reduce (the "late / partial peer" case)
void launch_xgmi_allreduce(float* grad, int64_t n, const XgmiPeers& P, int rank, int W, int64_t cap, int blocks,
                           uint64_t* seqs, float scale, unsigned* err, long long timeout_ticks,
                           const XgmiPostOpt* post, hipStream_t st, int fault = 0);
// The fused bf16 LeNet data-parallel step's view of the transport (lenet_mfma.hip, lenet_mwx):
// every gradient element the batch-reduction kernel produces is published as an 8-byte granule
// {fp32 value, low 32 bits of the block's launch counter} into its rank's granule array (parity
// p = seq & 1), written and read with single 8-byte system-scope accesses; a consumer lane polls the
// W - 1 peers' granules of ITS elements until their tags match, sums in rank order and applies the
// update in the same launch -- no flags, no barriers, one round trip. W = 1 is the loopback.
struct XgmiFused {
  uint64_t* gran[kXgmiMaxRanks];   // per-rank [2][cap] granules (indexed by flat parameter offset),
                                   // followed (gran + 2 cap) by the two-phase exchange's [2][cap] granules
                                   // of the REDUCED values of the 64-granule chunks the rank owns
                                   // (chunk c: rank c % W)
  uint64_t* seqs;                  // [G] per-block launch counters (this rank)
  unsigned* err;                   // sticky error word (host-mapped: the host polls it)
  unsigned* derr;                  // its device copy (what the kernel reads)
  int64_t cap;
  long long timeout;               // ticks of the 100 MHz constant clock
  int rank, W, G, fault;
  int two;                         // 1: two-phase exchange (reduce-scatter into owners, owners publish)
};
// two-shot variant: slot = floats per [rank] slot of t1 / t2 (>= ceil(n / W) rounded up to 4)
void launch_xgmi_allreduce_2shot(float* grad, int64_t n, const XgmiPeers& P, int rank, int W, int64_t slot,
                                 int blocks, uint64_t* seqs, float scale, unsigned* err, long long timeout_ticks,
                                 const XgmiPostOpt* post, hipStream_t st, int fault = 0);

int64_t colsum_ws_floats(int M, int N);
void launch_colsum_bf16(const uint16_t* X, int M, int N, int64_t ldx, float* out, int accumulate, float* ws,
                        hipStream_t st);
// out_k[c] (+)= sum_r part[r * ld + k * seg + c], c < W, k = 0..W/seg-1 (<= 3 segments; bit k of accmask =
// accumulate into out_k); fixed-order (deterministic)
struct SegOut {
  float* p[3];
};
void launch_reduce_rows(const float* part, int R, int64_t ld, int W, int seg, SegOut outs, int accmask, hipStream_t st);

// ----------------------------------------------------------------------------
// LayerNorm / embeddings (layernorm.hip), attention (attention.hip)
// ----------------------------------------------------------------------------
void launch_ln_fwd(const uint16_t* X, const float* gamma, const float* beta, uint16_t* Y, float* mean, float* rstd,
                   int64_t rows, int D, float eps, hipStream_t st);
int ln_bwd_partial_blocks(int64_t rows);
void launch_ln_bwd(const uint16_t* DY, const uint16_t* X, const float* gamma, const float* mean, const float* rstd,
                   uint16_t* DX, float* part, float* dgamma, float* dbeta, int64_t rows, int D, int accumulate,
                   const uint16_t* DRES, float* dxsum, int dxsum_acc, hipStream_t st);
// Hidden dropout (mlt_philox.h) fused into the LayerNorm kernels. Forward: Z = bf16(dropout(Y0) +
// RES), Y / mean / rstd = LayerNorm(Z). Backward: launch_ln_bwd's DX and partials, plus DXM =
// mask * scale * DX (the dY of the linear that produced Y0) whose column sums go to dxsum.
void launch_dropout_add_ln_fwd(const uint16_t* Y0, const uint16_t* RES, const float* gamma, const float* beta,
                               uint16_t* Z, uint16_t* Y, float* mean, float* rstd, int64_t rows, int D, float eps,
                               DropArgs dr, hipStream_t st);
void launch_ln_bwd_dropout(const uint16_t* DY, const uint16_t* X, const float* gamma, const float* mean,
                           const float* rstd, uint16_t* DX, uint16_t* DXM, float* part, float* dgamma, float* dbeta,
                           int64_t rows, int D, int accumulate, float* dxsum, int dxsum_acc, DropArgs dr,
                           hipStream_t st);
// Pre-norm blocks: the dropout variant with DRES added into DX (the residual stream's own gradient), the
// same kernel instantiation as launch_ln_bwd_dropout.
void launch_ln_bwd_dropout_res(const uint16_t* DY, const uint16_t* X, const float* gamma, const float* mean,
                               const float* rstd, uint16_t* DX, uint16_t* DXM, float* part, float* dgamma,
                               float* dbeta, int64_t rows, int D, int accumulate, const uint16_t* DRES, float* dxsum,
                               int dxsum_acc, DropArgs dr, hipStream_t st);
// RMSNorm (layernorm.hip): Y = bf16(x rstd g), rstd = rsqrt(mean(x^2) + eps) saved. The backward's part holds
// ln_bwd_partial_blocks(rows) * (dxsum ? 2 : 1) * D floats; DXM != nullptr (needs dxsum) is the dropout
// variant (dr is read then only); DRES may be given in every form.
void launch_rms_fwd(const uint16_t* X, const float* gamma, uint16_t* Y, float* rstd, int64_t rows, int D, float eps,
                    hipStream_t st);
void launch_dropout_add_rms_fwd(const uint16_t* Y0, const uint16_t* RES, const float* gamma, uint16_t* Z, uint16_t* Y,
                                float* rstd, int64_t rows, int D, float eps, DropArgs dr, hipStream_t st);
void launch_rms_bwd(const uint16_t* DY, const uint16_t* X, const float* gamma, const float* rstd, uint16_t* DX,
                    uint16_t* DXM, float* part, float* dgamma, int64_t rows, int D, int accumulate,
                    const uint16_t* DRES, float* dxsum, int dxsum_acc, DropArgs dr, hipStream_t st);
// out = keep ? bf16(x * scale) : 0 over numel (% 8 == 0) contiguous bf16 elements (dropout.hip)
void launch_dropout(const uint16_t* x, uint16_t* out, int64_t numel, DropArgs dr, hipStream_t st);
// pos (packed batches, or nullptr): the position of every row, each < S; nullptr: row % S.
// Wp == nullptr (rotary positions): out = word + type. launch_embed_bwd with gp == nullptr writes no
// position gradient.
void launch_embed_fwd(const int64_t* ids, const int64_t* tt, const uint16_t* Ww, const uint16_t* Wp,
                      const uint16_t* Wt, uint16_t* out, int64_t rows, int S, int D, int64_t vocab, int ntype,
                      hipStream_t st, const int* pos = nullptr);
// sid / perm: the token ids sorted stably and the sorting permutation (deterministic, atomic-free
// word-table scatter); part: S x 2D floats of per-position token-type partial sums. cu (packed
// batches, or nullptr): cu_seqlens [B + 1], sequence b = rows cu[b] .. cu[b + 1], each at most S long
void launch_embed_bwd(const int64_t* sid, const int64_t* perm, const int64_t* tt, const uint16_t* DX, float* gw,
                      float* gp, float* gt, float* part, int64_t rows, int S, int D, int64_t vocab, int ntype,
                      hipStream_t st, const int* cu = nullptr, int B = 0);
// One attention call: what the forward and the backward launchers agree on, besides their tensors.
struct AttnProblem {
  int B, S, H;  // batch, (maximum) sequence length, heads of 64 columns; D = 64 H
  float scale;
  // padded batch [B, S]: the valid length of every sequence (int32 [B] on the device, or nullptr: all S)
  const int* lens;
  // packed / unpadded batch, or nullptr: cu_seqlens [B + 1] on the device. qkv / out / dout / dqkv then
  // hold rows >= cu[B] token rows (sequence b at rows cu[b] .. cu[b + 1]; rows past cu[B] are untouched).
  // S is max_seqlen: it still sizes the grid, lse [B, H, S], the dropout tile stride and the column
  // partials. lens is unused. Ring kernels and bf16 outputs only.
  const int* cu;
  int rows;  // token rows of the packed tensors (unused without cu)
  // key j of a sequence is visible to query i of the same sequence iff j <= i and j < len_b (the CAUSAL
  // instantiations: the key / query loops stop at / start from the diagonal). Ring kernels and bf16
  // outputs only; composes with drop and cu.
  bool causal;
  // attention-probability dropout (mlt_philox.h): thr8 > 0 launches the dropout instantiations of the
  // forward and the two ring backward kernels; thr8 == 0 the plain ones
  AttnDropArgs drop;
};
void launch_attn_fwd(const AttnProblem& p, const uint16_t* qkv, uint16_t* out, float* lse, hipStream_t st);
// q8 (fp8 training, y != nullptr): instead of the bf16 dQKV, the backward kernels write its e5m2
// copy y [B*S][3D] and transpose yt [3D][B*S] -- each value the bf16 one rounded first, then scaled
// by *scale and quantised exactly as fp8_cast_transpose would -- and record amax(|dQKV|) into the
// kAmaxSlots sub-slots at amax (the ring kernels only; S % 16 == 0)
struct AttnQ8 {
  uint8_t* y = nullptr;
  uint8_t* yt = nullptr;
  const float* scale = nullptr;
  float* amax = nullptr;
  int64_t ldt = 0;  // yt row stride (B * S)
};
// Which backward kernels run a problem. attn_bwd_route decides it, from the problem, whether q8 outputs
// are asked for and the MLT_ATTN_* environment overrides, and raises every "no kernel for this
// combination" error (std::runtime_error): the caller routes before it allocates or launches anything.
struct AttnBwdRoute {
  bool ring;    // the ring kernels (the default), or the register-staged ones (MLT_ATTN_RING=0)
  bool k2, q2;  // 2 key / query groups (128 rows) per block in dK/dV / dQ, or 1 (64 rows)
  bool fullt;   // every 64-row stage is whole (padded, S % 64 == 0): the unclamped-row instantiations
  bool drop, packed, causal;
  // rows of column partials the ring kernels write: B x (row blocks of the chosen group count)
  int rows_q, rows_kv;
};
AttnBwdRoute attn_bwd_route(const AttnProblem& p, bool q8);
// colpart_q [rows_q][D] and colpart_kv [rows_kv][2D] (both or neither; ring kernels only): bias-gradient
// column partials of dQ and dK|dV. The register-staged kernels write none (the caller reduces dQKV itself).
void launch_attn_bwd(const AttnProblem& p, const AttnBwdRoute& r, const uint16_t* qkv, const uint16_t* out,
                     const uint16_t* dout, const float* lse, float* delta, uint16_t* dqkv, const AttnQ8& q8,
                     float* colpart_q, float* colpart_kv, hipStream_t st);
// Single-token attention over a key/value cache, append fused in (attn_decode.hip). qkv_new [B][ldq >= 3 * 64 H]
// (q | k | v of the B new tokens, ldq % 8 == 0, 16-byte aligned), kv [2][B][H][Smax][64] (keys, values), pos
// int32 [B] on the device (0 <= pos[b] < Smax: the row the new token takes = the tokens already cached),
// out [B][64 H]. Rows pos[b] of the cache are written, rows above are never read. rope (or nullptr: the kernel as
// it is without one): the rotary table [>= Smax][32][2] fp32; q and the new k are rotated by pos[b] and rounded to
// bf16 before the dot product and the append.
void launch_attn_decode(const uint16_t* qkv_new, int64_t ldq, uint16_t* kv, const int* pos, uint16_t* out, int B,
                        int H, int Smax, float scale, hipStream_t st, const float* rope = nullptr);
// Rotary position embedding of the q and k columns of qkv [rows][ld >= 3 * 64 H] in place (rope.hip): table
// [P][32][2] fp32 (cos, sin), the position of a row is pos[row] (int32 on the device, clamped into [0, P)) or,
// without pos, row % S (S <= P). sign >= 0: the rotation; < 0: the inverse rotation (its backward). ld % 8 == 0,
// 16-byte aligned base, rows * H * 8 < 2^31. The v columns and everything else are untouched.
void launch_rope_qk(uint16_t* qkv, int64_t ld, int64_t rows, int H, const float* table, int P, int S, const int* pos,
                    int sign, hipStream_t st);

// ----------------------------------------------------------------------------
// Masked-LM head (mlm.hip)
// ----------------------------------------------------------------------------
// vocab_ce: softmax cross-entropy over rows of bf16 logits Z[R, ldz] (ldz % 8 == 0, 16-byte aligned base,
// V <= ldz valid columns), one workgroup per row, the unscaled gradient softmax - onehot written in
// place when write_grad (padding columns and ignored rows as zeros). row_loss / row_lse / row_hit are
// fp32 [R], 0 for ignored rows. Rows of up to kVocabCeResidentCols columns stay in LDS between the
// statistics and the gradient write (one read of the logits); wider rows are read a second time.
constexpr int kVocabCeResidentCols = 31744;  // 62 KB of bf16: the 64 KB workgroup LDS less the reduction scratch
int vocab_ce_resident_cols();
void launch_vocab_ce(uint16_t* Z, int64_t R, int64_t ldz, int V, const int64_t* labels, float* row_loss,
                     float* row_lse, float* row_hit, int64_t ignore_index, bool write_grad, hipStream_t st);
// labels [B, S] -> P slots per sequence (slot_row int32 / slot_label int64, [R], R >= B * P; empty and
// tail slots -1 / ignore_index); lens [B] or cu [B + 1] (int32) or neither; seq_overflow [B], overflow [1].
void launch_mlm_select(const int64_t* labels, int B, int S, int P, int64_t R, const int* lens, const int* cu,
                       int64_t ignore_index, int* slot_row, int64_t* slot_label, int* seq_overflow, int* overflow,
                       hipStream_t st);
// out[R, h] = X[slot_row] (zeros for empty slots); dX[N, h] = 0 then dX[slot_row] = G. h % 8 == 0.
void launch_gather_rows(const uint16_t* X, int64_t N, int h, const int* slot_row, int64_t R, uint16_t* out,
                        hipStream_t st);
void launch_scatter_rows(const uint16_t* G, int64_t R, int h, const int* slot_row, int64_t N, uint16_t* dX,
                         hipStream_t st);

}  // namespace mlt
