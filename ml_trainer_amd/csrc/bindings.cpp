// Python bindings of the native extension ml_trainer_amd._C.
//
// Every launcher validates dtype/device/contiguity/shape on the host BEFORE the
// launch (a kernel that indexes past a buffer can take down the whole node), and
// launches on torch's current HIP stream so it composes with torch ops and with
// stream capture.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <torch/extension.h>

#include <cmath>
#include <map>
#include <memory>

#include "mlt_kernels.h"
#include "mlt_sample.h"
#include "mlt_comm.h"
#include "mlt_runtime.h"

namespace py = pybind11;
using at::Tensor;

namespace mlt {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

#define CHECK_CUDA_T(t) TORCH_CHECK((t).is_cuda(), #t " must be a device tensor")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHECK_F32(t) TORCH_CHECK((t).scalar_type() == at::kFloat, #t " must be float32")

static void check_dev(const Tensor& t, const char* name, at::ScalarType st, int64_t min_numel, int align = 16) {
  TORCH_CHECK(t.defined(), name, " is undefined");
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == st, name, " has dtype ", t.scalar_type(), ", expected ", st);
  TORCH_CHECK(t.numel() >= min_numel, name, " too small: ", t.numel(), " < ", min_numel);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0, name, " must be ", align, "-byte aligned");
}

// ----------------------------------------------------------------------------
// Flat optimizers
// ----------------------------------------------------------------------------
static OptHyper make_hyper(int kind, double lr, double momentum, double dampening, double wd, double beta1,
                           double beta2, double eps, double lr_decay, double grad_scale, bool nesterov,
                           bool maximize) {
  return make_opt_hyper(kind, lr, momentum, dampening, wd, beta1, beta2, eps, lr_decay, grad_scale, nesterov,
                        maximize);
}

void flat_optim(Tensor p, Tensor g, c10::optional<Tensor> s1, c10::optional<Tensor> s2, int kind, double lr,
                double momentum, double dampening, double wd, double beta1, double beta2, double eps,
                double lr_decay, double grad_scale, bool nesterov, bool maximize, c10::optional<Tensor> lr_t,
                c10::optional<Tensor> lr_index, c10::optional<Tensor> step_t, double t_host,
                c10::optional<Tensor> shadow, c10::optional<Tensor> coef) {
  const int64_t n = p.numel();
  TORCH_CHECK(n % 4 == 0, "flat buffer length must be a multiple of 4");
  check_dev(p, "p", at::kFloat, n);
  check_dev(g, "g", at::kFloat, n);
  TORCH_CHECK(kind >= 0 && kind <= 4, "unknown optimizer kind");
  const bool need_s2 = (kind == OPT_ADAM || kind == OPT_ADAMW || kind == OPT_ADAMAX);
  const bool need_s1 = need_s2 || kind == OPT_ADAGRAD || (kind == OPT_SGD && momentum != 0.0);
  float* s1p = nullptr;
  float* s2p = nullptr;
  if (need_s1) {
    TORCH_CHECK(s1.has_value(), "optimizer state s1 required");
    check_dev(*s1, "s1", at::kFloat, n);
    s1p = s1->data_ptr<float>();
  }
  if (need_s2) {
    TORCH_CHECK(s2.has_value(), "optimizer state s2 required");
    check_dev(*s2, "s2", at::kFloat, n);
    s2p = s2->data_ptr<float>();
  }
  const float* lrp = nullptr;
  const int64_t* lidx = nullptr;
  const int64_t* stp = nullptr;
  uint16_t* sh = nullptr;
  const float* cf = nullptr;
  if (lr_t.has_value()) {
    check_dev(*lr_t, "lr", at::kFloat, 1, 4);
    lrp = lr_t->data_ptr<float>();
  }
  if (lr_index.has_value()) {
    check_dev(*lr_index, "lr_index", at::kLong, 1, 8);
    lidx = lr_index->data_ptr<int64_t>();
  }
  if (step_t.has_value()) {
    check_dev(*step_t, "step", at::kLong, 1, 8);
    stp = step_t->data_ptr<int64_t>();
  }
  if (shadow.has_value()) {
    check_dev(*shadow, "shadow", at::kBFloat16, n);
    sh = reinterpret_cast<uint16_t*>(shadow->data_ptr());
  }
  if (coef.has_value()) {
    check_dev(*coef, "coef", at::kFloat, 1, 4);
    cf = coef->data_ptr<float>();
  }
  const OptHyper h = make_hyper(kind, lr, momentum, dampening, wd, beta1, beta2, eps, lr_decay, grad_scale,
                                nesterov, maximize);
  launch_flat_optim(p.data_ptr<float>(), g.data_ptr<float>(), s1p, s2p, n, h, lrp, lidx, stp, (float)t_host, sh,
                    cf, cur_stream());
}

// Arguments that flat_optim_seg and lamb_step share with flat_optim, checked the same way.
struct StepPtrs {
  const float* lr = nullptr;
  const int64_t* lr_index = nullptr;
  const int64_t* step = nullptr;
  uint16_t* shadow = nullptr;
  const float* coef = nullptr;
  const unsigned* skip = nullptr;
};

static StepPtrs step_ptrs(int64_t n, const c10::optional<Tensor>& lr_t, const c10::optional<Tensor>& lr_index,
                          const c10::optional<Tensor>& step_t, const c10::optional<Tensor>& shadow,
                          const c10::optional<Tensor>& coef, const c10::optional<Tensor>& skip) {
  StepPtrs s;
  if (lr_t.has_value()) {
    check_dev(*lr_t, "lr", at::kFloat, 1, 4);
    s.lr = lr_t->data_ptr<float>();
  }
  if (lr_index.has_value()) {
    TORCH_CHECK(lr_t.has_value(), "lr_index needs lr_t");
    check_dev(*lr_index, "lr_index", at::kLong, 1, 8);
    s.lr_index = lr_index->data_ptr<int64_t>();
  }
  if (step_t.has_value()) {
    check_dev(*step_t, "step", at::kLong, 1, 8);
    s.step = step_t->data_ptr<int64_t>();
  }
  if (shadow.has_value()) {
    check_dev(*shadow, "shadow", at::kBFloat16, n);
    s.shadow = reinterpret_cast<uint16_t*>(shadow->data_ptr());
  }
  if (coef.has_value()) {
    check_dev(*coef, "coef", at::kFloat, 1, 4);
    s.coef = coef->data_ptr<float>();
  }
  if (skip.has_value()) {
    check_dev(*skip, "skip", at::kInt, 1, 4);
    s.skip = reinterpret_cast<const unsigned*>(skip->data_ptr<int>());
  }
  return s;
}

// the flat buffers and the segment table; returns {nchunks, nt}
static std::pair<int, int> check_seg(const Tensor& p, const Tensor& g, const Tensor& s1, const Tensor& s2,
                                     const Tensor& chunks, const Tensor& wd) {
  const int64_t n = p.numel();
  TORCH_CHECK(n % 4 == 0, "flat buffer length must be a multiple of 4");
  TORCH_CHECK(n / 4 < (int64_t(1) << 31), "flat buffer too long for the 32-bit segment table");
  check_dev(p, "p", at::kFloat, n);
  check_dev(g, "g", at::kFloat, n);
  check_dev(s1, "s1", at::kFloat, n);
  check_dev(s2, "s2", at::kFloat, n);
  TORCH_CHECK(g.numel() == n && s1.numel() == n && s2.numel() == n, "p, g, s1, s2 must have one length");
  TORCH_CHECK(chunks.dim() == 2 && chunks.size(1) == 4, "chunks must be [nchunks, 4]");
  check_dev(chunks, "chunks", at::kInt, 0);
  TORCH_CHECK(wd.dim() == 1, "wd must be [tensors]");
  check_dev(wd, "wd", at::kFloat, 0, 4);
  TORCH_CHECK(chunks.size(0) < (int64_t(1) << 31) && wd.numel() < (int64_t(1) << 31), "segment table too long");
  return {(int)chunks.size(0), (int)wd.numel()};
}

void flat_optim_seg(Tensor p, Tensor g, Tensor s1, Tensor s2, Tensor chunks, Tensor wd, double lr, double beta1,
                    double beta2, double eps, double grad_scale, bool maximize, c10::optional<Tensor> lr_t,
                    c10::optional<Tensor> lr_index, c10::optional<Tensor> step_t, double t_host,
                    c10::optional<Tensor> shadow, c10::optional<Tensor> coef, c10::optional<Tensor> skip,
                    int max_blocks) {
  const auto [nchunks, nt] = check_seg(p, g, s1, s2, chunks, wd);
  const StepPtrs s = step_ptrs(p.numel(), lr_t, lr_index, step_t, shadow, coef, skip);
  const OptHyper h = make_hyper(OPT_ADAMW, lr, 0.0, 0.0, 0.0, beta1, beta2, eps, 0.0, grad_scale, false, maximize);
  launch_flat_optim_seg(p.data_ptr<float>(), g.data_ptr<float>(), s1.data_ptr<float>(), s2.data_ptr<float>(),
                        p.numel(), chunks.data_ptr<int>(), nchunks, wd.data_ptr<float>(), nt, h, s.lr, s.lr_index,
                        s.step, (float)t_host, s.shadow, s.coef, s.skip, max_blocks, cur_stream());
}

void lamb_step(Tensor p, Tensor g, Tensor m, Tensor v, Tensor chunks, Tensor tseg, Tensor wd, Tensor adapt,
               Tensor part, Tensor norms, Tensor trust, double lr, double beta1, double beta2, double eps,
               double grad_scale, bool maximize, c10::optional<Tensor> lr_t, c10::optional<Tensor> lr_index,
               c10::optional<Tensor> step_t, double t_host, c10::optional<Tensor> shadow,
               c10::optional<Tensor> coef, c10::optional<Tensor> skip, int max_blocks, int stages) {
  const auto [nchunks, nt] = check_seg(p, g, m, v, chunks, wd);
  TORCH_CHECK(tseg.dim() == 2 && tseg.size(0) == nt && tseg.size(1) == 2, "tseg must be [tensors, 2]");
  check_dev(tseg, "tseg", at::kInt, 0, 8);
  check_dev(adapt, "adapt", at::kInt, nt, 4);
  check_dev(part, "part", at::kFloat, 2 * (int64_t)nchunks, 8);
  check_dev(norms, "norms", at::kFloat, 2 * (int64_t)nt, 8);
  check_dev(trust, "trust", at::kFloat, nt, 4);
  TORCH_CHECK(stages >= 1 && stages <= 7, "stages is a mask of the three launches");
  const StepPtrs s = step_ptrs(p.numel(), lr_t, lr_index, step_t, shadow, coef, skip);
  const OptHyper h = make_hyper(OPT_LAMB, lr, 0.0, 0.0, 0.0, beta1, beta2, eps, 0.0, grad_scale, false, maximize);
  launch_lamb_step(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), p.numel(),
                   chunks.data_ptr<int>(), nchunks, tseg.data_ptr<int>(), wd.data_ptr<float>(),
                   adapt.data_ptr<int>(), nt, part.data_ptr<float>(), norms.data_ptr<float>(),
                   trust.data_ptr<float>(), h, s.lr, s.lr_index, s.step, (float)t_host, s.shadow, s.coef, s.skip,
                   max_blocks, stages, cur_stream());
}

void sq_norm(Tensor x, Tensor out) {
  TORCH_CHECK(x.numel() % 4 == 0, "sq_norm needs numel % 4 == 0");
  check_dev(x, "x", at::kFloat, x.numel());
  check_dev(out, "out", at::kFloat, 1, 4);
  // per-block partials (summed in block order by a second launch); stream-ordered scratch
  Tensor part = at::empty({sq_norm_partials_needed()}, x.options());
  launch_sq_norm(x.data_ptr<float>(), x.numel(), part.data_ptr<float>(), out.data_ptr<float>(), cur_stream());
}

void clip_coef(Tensor sq, double max_norm, Tensor coef, Tensor total) {
  check_dev(sq, "sq", at::kFloat, 1, 4);
  check_dev(coef, "coef", at::kFloat, 1, 4);
  check_dev(total, "total", at::kFloat, 1, 4);
  launch_clip_coef(sq.data_ptr<float>(), (float)max_norm, coef.data_ptr<float>(), total.data_ptr<float>(),
                   cur_stream());
}

void cast_bf16(Tensor x, Tensor y) {
  TORCH_CHECK(x.numel() % 4 == 0 && x.numel() == y.numel(), "cast_bf16 shape");
  check_dev(x, "x", at::kFloat, x.numel());
  check_dev(y, "y", at::kBFloat16, x.numel());
  launch_cast_bf16(x.data_ptr<float>(), reinterpret_cast<uint16_t*>(y.data_ptr()), x.numel(), cur_stream());
}

void transpose_bf16(Tensor src, Tensor dst) {
  TORCH_CHECK(src.dim() == 2 && dst.dim() == 2 && dst.size(0) == src.size(1) && dst.size(1) == src.size(0),
              "transpose_bf16: dst must be [C, R] for src [R, C]");
  check_dev(src, "src", at::kBFloat16, src.numel(), 2);
  check_dev(dst, "dst", at::kBFloat16, dst.numel(), 2);
  TORCH_CHECK(src.is_contiguous() && dst.is_contiguous(), "transpose_bf16: contiguous tensors");
  launch_transpose_bf16(reinterpret_cast<const uint16_t*>(src.data_ptr()), reinterpret_cast<uint16_t*>(dst.data_ptr()),
                        (int)src.size(0), (int)src.size(1), cur_stream());
}

// ----------------------------------------------------------------------------
// CIFAR device augmentation
// ----------------------------------------------------------------------------
static LeNetAug make_aug(const Tensor& data, const Tensor& perm, c10::optional<Tensor> ctrl, int64_t seed, int pad,
                         int flip, int batch_stride, const std::vector<double>& mean,
                         const std::vector<double>& stdv) {
  TORCH_CHECK(data.dim() == 4 && data.size(1) == 32 && data.size(2) == 32 && data.size(3) == 3,
              "data must be [N,32,32,3] uint8 (HWC)");
  check_dev(data, "data", at::kByte, data.numel());
  check_dev(perm, "perm", at::kInt, 1);
  TORCH_CHECK(mean.size() == 3 && stdv.size() == 3, "mean/std need 3 channels");
  TORCH_CHECK(pad >= 0 && pad <= 16, "pad out of range");
  LeNetAug A{};
  A.data = data.data_ptr<uint8_t>();
  A.perm = perm.data_ptr<int32_t>();
  A.ctrl = nullptr;
  if (ctrl.has_value()) {
    check_dev(*ctrl, "ctrl", at::kLong, 2, 8);
    A.ctrl = ctrl->data_ptr<int64_t>();
  }
  A.n = data.size(0);
  A.perm_len = perm.numel();
  A.seed = (uint64_t)seed;
  A.pad = pad;
  A.flip = flip;
  A.batch_stride = batch_stride;
  for (int c = 0; c < 3; ++c) {
    A.mean[c] = (float)mean[c];
    A.std[c] = (float)stdv[c];
    A.ascale[c] = (float)(1.0 / (255.0 * stdv[c]));  // (u / 255 - mean) / std = u * ascale + ashift
    A.ashift[c] = (float)(-mean[c] / stdv[c]);
  }
  return A;
}

void cifar_augment(Tensor data, Tensor perm, c10::optional<Tensor> ctrl, Tensor dtargets, Tensor out,
                   Tensor targets_out, int64_t seed, int pad, int flip, int batch_stride, std::vector<double> mean,
                   std::vector<double> stdv, int B, int64_t step_host, int64_t sie_host) {
  LeNetAug A = make_aug(data, perm, ctrl, seed, pad, flip, batch_stride, mean, stdv);
  A.step_host = step_host;
  A.sie_host = sie_host;
  TORCH_CHECK(B > 0, "B must be positive");
  check_dev(out, "out", at::kFloat, (int64_t)B * 3072);
  check_dev(targets_out, "targets_out", at::kLong, B);
  check_dev(dtargets, "dtargets", at::kLong, A.n);
  launch_cifar_augment(A, B, out.data_ptr<float>(), targets_out.data_ptr<int64_t>(), dtargets.data_ptr<int64_t>(),
                       cur_stream());
}

// ----------------------------------------------------------------------------
// Losses / metrics
// ----------------------------------------------------------------------------
static bool logits_bf16(const Tensor& z) {
  TORCH_CHECK(z.scalar_type() == at::kFloat || z.scalar_type() == at::kBFloat16, "logits must be fp32 or bf16");
  return z.scalar_type() == at::kBFloat16;
}

void ce_fwd(Tensor logits, Tensor tgt, Tensor dl, Tensor acc, c10::optional<Tensor> correct, Tensor loss,
            int64_t ignore_index, double label_smoothing) {
  TORCH_CHECK(logits.dim() == 2, "logits must be [B, C]");
  const int64_t B = logits.size(0), C = logits.size(1);
  const bool bf = logits_bf16(logits);
  check_dev(logits, "logits", logits.scalar_type(), B * C, 2);
  check_dev(tgt, "targets", at::kLong, B, 8);
  TORCH_CHECK(tgt.numel() == B, "targets must have B entries");
  check_dev(dl, "dl", at::kFloat, B * C, 4);
  check_dev(acc, "acc", at::kFloat, 2, 4);
  check_dev(loss, "loss", at::kFloat, 1, 4);
  float* cp = nullptr;
  if (correct.has_value()) {
    check_dev(*correct, "correct", at::kFloat, 1, 4);
    cp = correct->data_ptr<float>();
  }
  launch_ce_fwd(logits.data_ptr(), bf, tgt.data_ptr<int64_t>(), B, (int)C, dl.data_ptr<float>(),
                acc.data_ptr<float>(), cp, loss.data_ptr<float>(), ignore_index, (float)label_smoothing,
                cur_stream());
}

// BERT classifier layer (num_labels outputs): logits = pooled . W_c^T + b_c (fp32)
void head_cls_fwd(Tensor pooled, Tensor wc, c10::optional<Tensor> bc, Tensor logits) {
  TORCH_CHECK(pooled.dim() == 2 && wc.dim() == 2 && wc.size(1) == pooled.size(1), "head: pooled [B,h], W_c [L,h]");
  const int64_t B = pooled.size(0), h = pooled.size(1), L = wc.size(0);
  check_dev(pooled, "pooled", at::kFloat, B * h, 4);
  check_dev(wc, "W_c", at::kFloat, L * h, 4);
  if (bc.has_value()) check_dev(*bc, "b_c", at::kFloat, L, 4);
  check_dev(logits, "logits", at::kFloat, B * L, 4);
  launch_head_cls_fwd(pooled.data_ptr<float>(), (int)B, (int)h, wc.data_ptr<float>(),
                      bc.has_value() ? bc->data_ptr<float>() : nullptr, (int)L, logits.data_ptr<float>(), cur_stream());
}

// backward of the classifier layer + the pooler's tanh: dpre (bf16) and dW_c / db_c (fp32)
void head_cls_bwd(Tensor dlogits, Tensor pooled, Tensor wc, Tensor dpre, Tensor dwc, c10::optional<Tensor> dbc,
                  bool accumulate) {
  const int64_t B = pooled.size(0), h = pooled.size(1), L = wc.size(0);
  check_dev(dlogits, "dlogits", at::kFloat, B * L, 4);
  check_dev(pooled, "pooled", at::kFloat, B * h, 4);
  check_dev(wc, "W_c", at::kFloat, L * h, 4);
  check_dev(dpre, "dpre", at::kBFloat16, B * h, 2);
  check_dev(dwc, "dW_c", at::kFloat, L * h, 4);
  TORCH_CHECK(L >= 1 && L <= 1024, "head backward: num_labels must be in [1, 1024]");
  if (dbc.has_value()) check_dev(*dbc, "db_c", at::kFloat, L, 4);
  launch_head_cls_bwd(dlogits.data_ptr<float>(), pooled.data_ptr<float>(), wc.data_ptr<float>(), (int)B, (int)h,
                      (int)L, (uint16_t*)dpre.data_ptr(), dwc.data_ptr<float>(),
                      dbc.has_value() ? dbc->data_ptr<float>() : nullptr, accumulate, cur_stream());
}

void ce_bwd(Tensor dl, Tensor gout, Tensor acc, Tensor out) {
  check_dev(dl, "dl", at::kFloat, dl.numel(), 4);
  check_dev(gout, "grad_out", at::kFloat, 1, 4);
  check_dev(acc, "acc", at::kFloat, 2, 4);
  TORCH_CHECK(out.numel() == dl.numel(), "out size");
  const bool bf = logits_bf16(out);
  check_dev(out, "out", out.scalar_type(), dl.numel(), 2);
  launch_ce_bwd(dl.data_ptr<float>(), gout.data_ptr<float>(), acc.data_ptr<float>(), dl.numel(), out.data_ptr(),
                bf, cur_stream());
}

void accuracy(Tensor logits, Tensor tgt, Tensor out) {
  TORCH_CHECK(logits.dim() == 2, "logits must be [B, C]");
  const int64_t B = logits.size(0), C = logits.size(1);
  const bool bf = logits_bf16(logits);
  check_dev(logits, "logits", logits.scalar_type(), B * C, 2);
  check_dev(tgt, "targets", at::kLong, B, 8);
  TORCH_CHECK(tgt.numel() == B, "targets must have B entries");
  check_dev(out, "out", at::kFloat, 1, 4);
  launch_accuracy(logits.data_ptr(), bf, tgt.data_ptr<int64_t>(), B, (int)C, out.data_ptr<float>(), cur_stream());
}

void pointwise_loss_fwd(Tensor p, Tensor t, int64_t mode, Tensor g, Tensor part, Tensor out) {
  const int64_t n = p.numel();
  TORCH_CHECK(mode == 0 || mode == 1, "mode must be 0 (l1) or 1 (mse)");
  TORCH_CHECK(t.numel() == n && g.numel() == n, "pred/target/grad sizes differ");
  check_dev(p, "pred", at::kFloat, n, 4);
  check_dev(t, "target", at::kFloat, n, 4);
  check_dev(g, "grad", at::kFloat, n, 4);
  check_dev(part, "partials", at::kFloat, loss_partials_needed(), 4);
  check_dev(out, "out", at::kFloat, 2, 4);
  launch_pointwise_loss_fwd(p.data_ptr<float>(), t.data_ptr<float>(), n, (int)mode, g.data_ptr<float>(),
                            part.data_ptr<float>(), out.data_ptr<float>(), cur_stream());
}

void nll_fwd(Tensor logp, Tensor tgt, int64_t ignore_index, Tensor part, Tensor out) {
  TORCH_CHECK(logp.dim() == 2, "log-probabilities must be [B, C]");
  const int64_t B = logp.size(0), C = logp.size(1);
  check_dev(logp, "logp", at::kFloat, B * C, 4);
  check_dev(tgt, "targets", at::kLong, B, 8);
  TORCH_CHECK(tgt.numel() == B, "targets must have B entries");
  check_dev(part, "partials", at::kFloat, loss_partials_needed(), 4);
  check_dev(out, "out", at::kFloat, 2, 4);
  launch_nll_fwd(logp.data_ptr<float>(), tgt.data_ptr<int64_t>(), B, (int)C, ignore_index, part.data_ptr<float>(),
                 out.data_ptr<float>(), cur_stream());
}

void loss_scale_grad(Tensor g, Tensor gout, Tensor stats, Tensor out) {
  const int64_t n = g.numel();
  check_dev(g, "g", at::kFloat, n, 4);
  check_dev(gout, "grad_out", at::kFloat, 1, 4);
  check_dev(stats, "stats", at::kFloat, 2, 4);
  TORCH_CHECK(out.numel() == n, "out size");
  check_dev(out, "out", at::kFloat, n, 4);
  launch_loss_scale_grad(g.data_ptr<float>(), gout.data_ptr<float>(), stats.data_ptr<float>(), n,
                         out.data_ptr<float>(), cur_stream());
}

void nll_bwd(Tensor tgt, int64_t C, int64_t ignore_index, Tensor gout, Tensor stats, Tensor out) {
  const int64_t B = tgt.numel();
  check_dev(tgt, "targets", at::kLong, B, 8);
  check_dev(gout, "grad_out", at::kFloat, 1, 4);
  check_dev(stats, "stats", at::kFloat, 2, 4);
  TORCH_CHECK(out.numel() == B * C, "out size");
  check_dev(out, "out", at::kFloat, B * C, 4);
  launch_nll_bwd(tgt.data_ptr<int64_t>(), B, (int)C, ignore_index, gout.data_ptr<float>(), stats.data_ptr<float>(),
                 out.data_ptr<float>(), cur_stream());
}

void mcrmse(Tensor p, Tensor t, Tensor col, Tensor out) {
  TORCH_CHECK(p.dim() == 2 && t.sizes() == p.sizes(), "mcrmse expects matching [B, C] tensors");
  const int64_t B = p.size(0), C = p.size(1);
  check_dev(p, "pred", at::kFloat, B * C, 4);
  check_dev(t, "target", at::kFloat, B * C, 4);
  check_dev(col, "col", at::kFloat, C, 4);
  check_dev(out, "out", at::kFloat, 1, 4);
  launch_mcrmse(p.data_ptr<float>(), t.data_ptr<float>(), B, (int)C, col.data_ptr<float>(), out.data_ptr<float>(),
                cur_stream());
}

// ----------------------------------------------------------------------------
// bf16 GEMM
// ----------------------------------------------------------------------------
static const uint16_t* bf16_ptr(const Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
// a forced GEMM configuration: 6 was the persistent ping-pong kernel, whose number stays unused
static void check_gemm_cfg(int cfg) {
  TORCH_CHECK(cfg != 6, "GEMM configuration 6 (persistent ping-pong) was retired; use 5 (ping-pong) or 7 (4-wave)");
}

// One matrix operand of a GEMM binding: 2-D, on the device, unit column stride, a row stride that is a
// multiple of row_mult (0: not checked for this operand) and a 16-byte aligned base. `name` is the
// binding's; the other texts are the binding's own wording of the condition.
struct GemmOperandText {
  const char *name, *device, *col_stride, *row_stride;
};
static void check_gemm_operand(const Tensor& t, const GemmOperandText& tx, int64_t row_mult) {
  TORCH_CHECK(t.dim() == 2, tx.name, " operands must be 2-D");
  TORCH_CHECK(t.is_cuda(), tx.device);
  TORCH_CHECK(t.stride(1) == 1, tx.col_stride);
  TORCH_CHECK(row_mult == 0 || t.stride(0) % row_mult == 0, tx.row_stride);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, tx.name, " operands must be 16-byte aligned");
}

// The epilogue side operands of a GEMM with an [M, N] output: fp32 bias [N], the bf16 [M, N] GELU
// pre-activation aux (modes 1 gelu / 2 dgelu; strict_aux: with row stride % 8 == 0 and a 16-byte base as
// well) and the bf16 [M, N] residual res. no_aux / bad_aux: the binding's texts for a missing / unfit aux.
struct GemmEpiOperands {
  const float* bias = nullptr;
  const uint16_t* aux = nullptr;
  const uint16_t* res = nullptr;
  int64_t ldaux = 0, ldres = 0;
};
static GemmEpiOperands check_gemm_epilogue(const c10::optional<Tensor>& bias, const c10::optional<Tensor>& aux,
                                           const c10::optional<Tensor>& res, int64_t M, int64_t N, int mode,
                                           bool strict_aux, const char* no_aux, const char* bad_aux) {
  const auto bf16_mn = [&](const Tensor& t) {
    return t.scalar_type() == at::kBFloat16 && t.dim() == 2 && t.size(0) == M && t.size(1) == N && t.stride(1) == 1 &&
           t.is_cuda();
  };
  GemmEpiOperands e;
  if (bias.has_value()) {
    check_dev(*bias, "bias", at::kFloat, N, 4);
    e.bias = bias->data_ptr<float>();
  }
  if (mode == 1 || mode == 2) {  // GELU writes / dGELU reads the pre-activation (tanh needs none)
    TORCH_CHECK(aux.has_value(), no_aux);
    TORCH_CHECK(bf16_mn(*aux) && (!strict_aux || (aux->stride(0) % 8 == 0 &&
                                                   reinterpret_cast<uintptr_t>(aux->data_ptr()) % 16 == 0)),
                bad_aux);
    e.aux = bf16_ptr(*aux);
    e.ldaux = aux->stride(0);
  }
  if (res.has_value()) {
    TORCH_CHECK(bf16_mn(*res), "res must be bf16 [M,N]");
    e.res = bf16_ptr(*res);
    e.ldres = res->stride(0);
  }
  return e;
}

// colsum_out[n] (+)= the sum over the rows of part [rows, N]: the column partials a kernel's epilogue
// left (per 64 or 128 output rows) become the bias gradient, in a fixed order
static void reduce_col_partials(const Tensor& part, int64_t rows, int64_t N, float* colsum_out, bool accumulate) {
  SegOut o{{colsum_out, nullptr, nullptr}};
  launch_reduce_rows(part.data_ptr<float>(), (int)rows, N, (int)N, (int)N, o, accumulate ? 1 : 0, cur_stream());
}

// A, B, C are 2-D (row-major, unit column stride). a_mn / b_mn describe the storage:
//   A: [M,K] (a_mn=0) or [K,M] (a_mn=1);  B: [N,K] (b_mn=0) or [K,N] (b_mn=1);  C: [M,N].
void gemm(Tensor A, Tensor B, Tensor C, bool a_mn, bool b_mn, c10::optional<Tensor> bias, c10::optional<Tensor> aux,
          c10::optional<Tensor> res, double alpha, int mode, bool accumulate, int cfg, int splits,
          c10::optional<Tensor> colsum_out, bool colsum_accumulate) {
  check_gemm_cfg(cfg);
  static const GemmOperandText tx{"gemm", "gemm operands must be device tensors",
                                  "gemm operands need unit column stride",
                                  "gemm leading dimensions must be multiples of 8"};
  check_gemm_operand(A, tx, 8);
  check_gemm_operand(B, tx, 8);
  check_gemm_operand(C, tx, 0);
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 && B.scalar_type() == at::kBFloat16, "gemm A/B must be bf16");
  TORCH_CHECK(C.scalar_type() == at::kBFloat16 || C.scalar_type() == at::kFloat, "gemm C must be bf16 or fp32");
  const int64_t M = a_mn ? A.size(1) : A.size(0), K = a_mn ? A.size(0) : A.size(1);
  const int64_t N = b_mn ? B.size(1) : B.size(0), K2 = b_mn ? B.size(0) : B.size(1);
  TORCH_CHECK(K == K2, "gemm inner dimensions differ: ", K, " vs ", K2);
  TORCH_CHECK(C.size(0) == M && C.size(1) == N, "gemm C shape mismatch");
  // 16-byte chunks along the contiguous dimension of each operand
  TORCH_CHECK((a_mn ? M : K) % 8 == 0 && (b_mn ? N : K) % 8 == 0, "contiguous gemm dims must be multiples of 8");
  TORCH_CHECK(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), "gemm dims too large");
  TORCH_CHECK(mode >= 0 && mode <= 3, "gemm mode (0 none, 1 gelu, 2 dgelu, 3 tanh)");
  const GemmEpiOperands ep =
      check_gemm_epilogue(bias, aux, res, M, N, mode, false, "gemm GELU modes need aux", "aux must be bf16 [M,N]");
  TORCH_CHECK(!accumulate || C.scalar_type() == at::kFloat, "accumulate needs an fp32 output");
  Tensor part;
  if (colsum_out.has_value()) {
    // column sums of the dGELU output (the bias gradient of the layer that produced aux) from the
    // ping-pong kernel's epilogue: every tile must take its dGELU side-operand pass
    TORCH_CHECK(mode == 2 && !res.has_value() && !accumulate && C.scalar_type() == at::kBFloat16 && !a_mn,
                "colsum_out: dGELU mode, bf16 output, k-contiguous A, no residual / accumulate");
    TORCH_CHECK(M % 256 == 0 && N % 256 == 0 && K % 64 == 0 && C.stride(0) % 8 == 0 && ep.ldaux % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(ep.aux) % 16 == 0,
                "colsum_out needs M % 256 == 0, N % 256 == 0, K % 64 == 0 and 16-byte aligned rows of C / aux");
    check_dev(*colsum_out, "colsum_out", at::kFloat, N, 16);
    // the 4-wave kernel (cfg 7) when the planner takes it (its epilogue writes the same per-64-row
    // partials), else the ping-pong tile
    if (cfg != 7 && !(cfg < 0 && plan_gemm_bf16(a_mn, b_mn, (int)M, (int)N, (int)K, -1, 0).cfg == 7)) cfg = 5;
    else cfg = 7;
    splits = 1;
    part = at::empty({M / 64 * N}, A.options().dtype(at::kFloat));
  }
  const GemmPlan plan = plan_gemm_bf16(a_mn, b_mn, (int)M, (int)N, (int)K, cfg, splits, accumulate ? 1 : 0);
  TORCH_CHECK(!part.defined() || ((plan.cfg == 5 || plan.cfg == 7) && plan.splits == 1),
              "colsum_out: ping-pong / 4-wave plan expected");
  Tensor ws;
  if (plan.ws_floats > 0) ws = at::empty({plan.ws_floats}, A.options().dtype(at::kFloat));
  launch_gemm_bf16(plan, a_mn, b_mn, C.scalar_type() == at::kFloat, bf16_ptr(A), bf16_ptr(B), C.data_ptr(), (int)M,
                   (int)N, (int)K, A.stride(0), B.stride(0), C.stride(0), ep.bias, ep.aux, ep.ldaux, ep.res, ep.ldres,
                   (float)alpha, mode, accumulate ? 1 : 0, ws.defined() ? ws.data_ptr<float>() : nullptr, nullptr,
                   cur_stream(), part.defined() ? part.data_ptr<float>() : nullptr);
  if (part.defined()) reduce_col_partials(part, M / 64, N, colsum_out->data_ptr<float>(), colsum_accumulate);
}

// Y [M, N] = epilogue(X [M, K] . W [N, K]^T) on the weight-streaming kernel of the decode steps (gemm_skinny.hip):
// 1 <= M <= gemm_skinny_max_rows(), N % 16 == 0, K % 32 == 0, mode 0 (none) or 1 (GELU, aux receives the
// pre-activation). Everything else is refused here: there is no fall-back to another kernel.
void gemm_skinny(Tensor X, Tensor W, Tensor Y, c10::optional<Tensor> bias, c10::optional<Tensor> aux,
                 c10::optional<Tensor> res, int mode) {
  static const GemmOperandText tx{"gemm_skinny", "gemm_skinny operands must be device tensors",
                                  "gemm_skinny operands need unit column stride (k-contiguous X and W)",
                                  "gemm_skinny leading dimensions must be multiples of 8"};
  check_gemm_operand(X, tx, 8);
  check_gemm_operand(W, tx, 8);
  check_gemm_operand(Y, tx, 0);
  TORCH_CHECK(X.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16, "gemm_skinny X/W must be bf16");
  TORCH_CHECK(Y.scalar_type() == at::kBFloat16 || Y.scalar_type() == at::kFloat, "gemm_skinny Y must be bf16 or fp32");
  const int64_t M = X.size(0), K = X.size(1), N = W.size(0);
  TORCH_CHECK(W.size(1) == K, "gemm_skinny inner dimensions differ: ", K, " vs ", W.size(1));
  TORCH_CHECK(Y.size(0) == M && Y.size(1) == N, "gemm_skinny Y shape mismatch");
  TORCH_CHECK(M >= 1 && M <= kSkinnyMaxRows, "gemm_skinny takes 1 .. ", kSkinnyMaxRows, " rows, got ", M);
  TORCH_CHECK(N % 16 == 0 && K % 32 == 0 && N > 0 && K > 0, "gemm_skinny needs N % 16 == 0 and K % 32 == 0, got N = ", N,
              ", K = ", K);
  TORCH_CHECK(N < (1LL << 31) && K < (1LL << 31), "gemm_skinny dims too large");
  TORCH_CHECK(mode == 0 || mode == 1, "gemm_skinny mode (0 none, 1 gelu); dgelu / tanh run on gemm");
  TORCH_CHECK(X.stride(0) >= K && W.stride(0) >= K && Y.stride(0) >= N, "gemm_skinny rows overlap");
  const GemmEpiOperands ep = check_gemm_epilogue(bias, aux, res, M, N, mode, true, "gemm_skinny GELU mode needs aux",
                                                 "aux must be bf16 [M,N] with 16-byte aligned rows");
  launch_gemm_skinny(bf16_ptr(X), bf16_ptr(W), Y.data_ptr(), Y.scalar_type() == at::kFloat, (int)M, (int)N, (int)K,
                     X.stride(0), W.stride(0), Y.stride(0), ep.bias, ep.aux, ep.ldaux, ep.res, ep.ldres, mode,
                     cur_stream());
}

// ---------------------------------------------------------------------------- fp8
static bool is_fp8_storage(const Tensor& t) {
  return t.scalar_type() == at::kByte || t.scalar_type() == at::kFloat8_e4m3fn ||
         t.scalar_type() == at::kFloat8_e5m2;
}
static const uint8_t* u8(const Tensor& t) { return reinterpret_cast<const uint8_t*>(t.data_ptr()); }

void gemm_f8(Tensor A, Tensor B, Tensor C, int fmt_a, int fmt_b, Tensor inv_scale_a, Tensor inv_scale_b,
             c10::optional<Tensor> bias, c10::optional<Tensor> aux, c10::optional<Tensor> res, double alpha, int mode,
             bool accumulate, int cfg, int splits) {
  check_gemm_cfg(cfg);
  static const char* const text = "gemm_f8 operands: device tensors with unit column stride";
  static const GemmOperandText tx{"gemm_f8", text, text, "gemm_f8 row strides must be multiples of 16"};
  check_gemm_operand(A, tx, 16);
  check_gemm_operand(B, tx, 16);
  check_gemm_operand(C, tx, 0);
  TORCH_CHECK(is_fp8_storage(A) && is_fp8_storage(B), "gemm_f8 A/B must be fp8 (or uint8) storage");
  TORCH_CHECK((fmt_a == 0 || fmt_a == 1) && (fmt_b == 0 || fmt_b == 1) && !(fmt_a == 1 && fmt_b == 1),
              "fp8 formats: 0 = e4m3, 1 = e5m2 (e5m2 x e5m2 not supported)");
  TORCH_CHECK(C.scalar_type() == at::kBFloat16 || C.scalar_type() == at::kFloat, "gemm_f8 C must be bf16 or fp32");
  const int64_t M = A.size(0), K = A.size(1), N = B.size(0);
  TORCH_CHECK(B.size(1) == K, "gemm_f8 inner dimensions differ");
  TORCH_CHECK(C.size(0) == M && C.size(1) == N, "gemm_f8 C shape mismatch");
  TORCH_CHECK(K % 128 == 0 && M >= 64 && N >= 64, "gemm_f8 needs K % 128 == 0 and M, N >= 64");
  check_dev(inv_scale_a, "inv_scale_a", at::kFloat, 1, 4);
  check_dev(inv_scale_b, "inv_scale_b", at::kFloat, 1, 4);
  TORCH_CHECK(mode >= 0 && mode <= 3, "gemm mode (0 none, 1 gelu, 2 dgelu, 3 tanh)");
  static const char* const aux_text = "gemm_f8 mode 1/2: aux must be bf16 [M,N]";
  const GemmEpiOperands ep = check_gemm_epilogue(bias, aux, res, M, N, mode, false, aux_text, aux_text);
  TORCH_CHECK(!accumulate || C.scalar_type() == at::kFloat, "accumulate needs an fp32 output");
  const GemmPlan plan = plan_gemm_f8((int)M, (int)N, (int)K, cfg, splits);
  TORCH_CHECK(plan.cfg >= 1, "no fp8 GEMM configuration for this shape");
  Tensor ws;
  if (plan.ws_floats > 0) ws = at::empty({plan.ws_floats}, C.options().dtype(at::kFloat));
  launch_gemm_f8(plan, fmt_a, fmt_b, C.scalar_type() == at::kFloat, u8(A), u8(B), C.data_ptr(), (int)M, (int)N,
                 (int)K, A.stride(0), B.stride(0), C.stride(0), inv_scale_a.data_ptr<float>(),
                 inv_scale_b.data_ptr<float>(), ep.bias, ep.aux, ep.ldaux, ep.res, ep.ldres, (float)alpha, mode,
                 accumulate ? 1 : 0, ws.defined() ? ws.data_ptr<float>() : nullptr, nullptr, cur_stream());
}

// fp8 GEMM whose epilogue quantises its own output: Y (fp8 [M,N]) and Yt (fp8 [N,M]) for the
// consumer GEMMs, amax into out_amax, and (colsum_out) the column sums of the unquantised output
void gemm_f8_q(Tensor A, Tensor B, Tensor Y, Tensor Yt, int fmt_a, int fmt_b, Tensor inv_scale_a, Tensor inv_scale_b,
               int out_fmt, Tensor out_scale, Tensor out_amax, c10::optional<Tensor> bias, c10::optional<Tensor> aux,
               int mode, c10::optional<Tensor> colsum_out, bool colsum_accumulate) {
  static const char* const text = "gemm_f8_q operands: device tensors, unit column stride, row stride % 16 == 0";
  static const GemmOperandText tx{"gemm_f8_q", text, text, text};
  for (const Tensor* t : {&A, &B, &Y, &Yt}) check_gemm_operand(*t, tx, 16);
  TORCH_CHECK(is_fp8_storage(A) && is_fp8_storage(B) && is_fp8_storage(Y) && is_fp8_storage(Yt),
              "gemm_f8_q A/B/Y/Yt must be fp8 (or uint8) storage");
  TORCH_CHECK((fmt_a == 0 || fmt_a == 1) && fmt_b == 0, "gemm_f8_q formats: A e4m3/e5m2, B e4m3");
  TORCH_CHECK(out_fmt == 0 || out_fmt == 1, "out_fmt: 0 = e4m3, 1 = e5m2");
  const int64_t M = A.size(0), K = A.size(1), N = B.size(0);
  TORCH_CHECK(B.size(1) == K, "gemm_f8_q inner dimensions differ");
  TORCH_CHECK(M % 256 == 0 && N % 256 == 0 && K % 128 == 0 && K > 0,
              "gemm_f8_q needs M % 256 == 0, N % 256 == 0, K % 128 == 0");
  TORCH_CHECK(Y.size(0) == M && Y.size(1) == N && Yt.size(0) == N && Yt.size(1) == M, "gemm_f8_q Y / Yt shapes");
  check_dev(inv_scale_a, "inv_scale_a", at::kFloat, 1, 4);
  check_dev(inv_scale_b, "inv_scale_b", at::kFloat, 1, 4);
  check_dev(out_scale, "out_scale", at::kFloat, 1, 4);
  check_dev(out_amax, "out_amax", at::kFloat, kAmaxSlots * kAmaxStride, 4);
  TORCH_CHECK(mode >= 0 && mode <= 2, "gemm_f8_q mode (0 none, 1 gelu, 2 dgelu)");
  static const char* const aux_text = "aux must be a 16-byte aligned bf16 [M,N] with row stride % 8 == 0";
  const GemmEpiOperands ep = check_gemm_epilogue(bias, aux, c10::nullopt, M, N, mode, true, aux_text, aux_text);
  Tensor part;
  if (colsum_out.has_value()) {
    check_dev(*colsum_out, "colsum_out", at::kFloat, N, 16);
    part = at::empty({M / 64 * N}, A.options().dtype(at::kFloat));
  }
  launch_gemm_f8_q(fmt_a, fmt_b, u8(A), u8(B), reinterpret_cast<uint8_t*>(Y.data_ptr()),
                   reinterpret_cast<uint8_t*>(Yt.data_ptr()), (int)M, (int)N, (int)K, A.stride(0), B.stride(0),
                   Y.stride(0), Yt.stride(0), inv_scale_a.data_ptr<float>(), inv_scale_b.data_ptr<float>(), ep.bias,
                   ep.aux, ep.ldaux, mode, out_fmt, out_scale.data_ptr<float>(), out_amax.data_ptr<float>(),
                   part.defined() ? part.data_ptr<float>() : nullptr, cur_stream());
  if (part.defined()) reduce_col_partials(part, M / 64, N, colsum_out->data_ptr<float>(), colsum_accumulate);
}

void fp8_cast(Tensor x, Tensor y, Tensor scale, c10::optional<Tensor> amax, int fmt) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat),
              "fp8_cast x: contiguous bf16/fp32 device tensor");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() && is_fp8_storage(y) && y.numel() == x.numel(), "fp8_cast y");
  TORCH_CHECK(x.numel() % 8 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(y.data_ptr()) % 8 == 0, "fp8_cast needs numel % 8 == 0 and aligned data");
  check_dev(scale, "scale", at::kFloat, 1, 4);
  float* am = nullptr;
  if (amax.has_value()) {
    check_dev(*amax, "amax", at::kFloat, kAmaxSlots * kAmaxStride, 4);
    am = amax->data_ptr<float>();
  }
  launch_cast_fp8(x.data_ptr(), x.scalar_type() == at::kFloat, reinterpret_cast<uint8_t*>(y.data_ptr()), x.numel(),
                  scale.data_ptr<float>(), am, fmt, cur_stream());
}

void fp8_amax(Tensor x, Tensor amax) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat),
              "fp8_amax x");
  TORCH_CHECK(x.numel() % 8 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "fp8_amax alignment");
  check_dev(amax, "amax", at::kFloat, kAmaxSlots * kAmaxStride, 4);
  launch_amax(x.data_ptr(), x.scalar_type() == at::kFloat, x.numel(), amax.data_ptr<float>(), cur_stream());
}

void fp8_cast_transpose(Tensor w, Tensor y, Tensor yt, Tensor scale, c10::optional<Tensor> amax, int fmt,
                        c10::optional<Tensor> colsum_out, bool colsum_accumulate) {
  TORCH_CHECK(w.dim() == 2 && w.is_cuda() && w.is_contiguous() &&
                  (w.scalar_type() == at::kFloat || w.scalar_type() == at::kBFloat16),
              "w: fp32 or bf16 [R,C]");
  const int64_t R = w.size(0), Cc = w.size(1);
  TORCH_CHECK(R % 4 == 0 && Cc % 4 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0, "w shape/alignment");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() && is_fp8_storage(y) && y.numel() == R * Cc, "y");
  TORCH_CHECK(yt.is_cuda() && yt.is_contiguous() && is_fp8_storage(yt) && yt.numel() == R * Cc, "yt");
  // the 64x64 kernel stores dwords to both (the wide one 8 bytes, which cast_transpose_fp8_wide_ok checks itself)
  TORCH_CHECK(reinterpret_cast<uintptr_t>(y.data_ptr()) % 4 == 0 && reinterpret_cast<uintptr_t>(yt.data_ptr()) % 4 == 0,
              "fp8_cast_transpose y / yt must be 4-byte aligned");
  check_dev(scale, "scale", at::kFloat, 1, 4);
  float* am = nullptr;
  if (amax.has_value()) {
    check_dev(*amax, "amax", at::kFloat, kAmaxSlots * kAmaxStride, 4);
    am = amax->data_ptr<float>();
  }
  TORCH_CHECK(fmt == 0 || fmt == 1, "fmt: 0 = e4m3, 1 = e5m2");
  TORCH_CHECK(!colsum_out.has_value() || w.scalar_type() == at::kBFloat16, "colsum_out needs a bf16 input");
  if (w.scalar_type() == at::kFloat)
    launch_cast_transpose_fp8(w.data_ptr<float>(), reinterpret_cast<uint8_t*>(y.data_ptr()),
                              reinterpret_cast<uint8_t*>(yt.data_ptr()), (int)R, (int)Cc, scale.data_ptr<float>(), am,
                              fmt, cur_stream());
  else if (!colsum_out.has_value())
    launch_cast_transpose_fp8_bf16(bf16_ptr(w), reinterpret_cast<uint8_t*>(y.data_ptr()),
                                   reinterpret_cast<uint8_t*>(yt.data_ptr()), (int)R, (int)Cc, scale.data_ptr<float>(),
                                   am, fmt, cur_stream());
  else {
    // column sums of w (the bias gradient when w is a GEMM's dY) from the same read of w
    check_dev(*colsum_out, "colsum_out", at::kFloat, Cc, 16);
    float* cs = colsum_out->data_ptr<float>();
    const int acc = colsum_accumulate ? 1 : 0;
    if (cast_transpose_fp8_wide_ok(w.data_ptr(), y.data_ptr(), yt.data_ptr(), (int)R, (int)Cc)) {
      Tensor ws = at::empty({R / 128 * Cc}, w.options().dtype(at::kFloat));
      launch_cast_transpose_fp8_bf16(bf16_ptr(w), reinterpret_cast<uint8_t*>(y.data_ptr()),
                                     reinterpret_cast<uint8_t*>(yt.data_ptr()), (int)R, (int)Cc,
                                     scale.data_ptr<float>(), am, fmt, cur_stream(), ws.data_ptr<float>());
      reduce_col_partials(ws, R / 128, Cc, cs, colsum_accumulate);
    } else {
      launch_cast_transpose_fp8_bf16(bf16_ptr(w), reinterpret_cast<uint8_t*>(y.data_ptr()),
                                     reinterpret_cast<uint8_t*>(yt.data_ptr()), (int)R, (int)Cc,
                                     scale.data_ptr<float>(), am, fmt, cur_stream());
      Tensor ws = at::empty({std::max<int64_t>(colsum_ws_floats((int)R, (int)Cc), 4)}, w.options().dtype(at::kFloat));
      launch_colsum_bf16(bf16_ptr(w), (int)R, (int)Cc, Cc, cs, acc, ws.data_ptr<float>(), cur_stream());
    }
  }
}

// hist [n, H], amax [n, kAmaxSlots], scale / inv_scale / fmax [n]
void fp8_update_scale(Tensor hist, Tensor amax, Tensor scale, Tensor inv_scale, Tensor fmax, int64_t step,
                      int margin) {
  TORCH_CHECK(hist.dim() == 2 && hist.is_contiguous(), "hist must be [n, H]");
  const int64_t n_slots = amax.numel();
  TORCH_CHECK(n_slots % (kAmaxSlots * kAmaxStride) == 0, "amax must be [n, ", kAmaxSlots * kAmaxStride, "]");
  const int64_t nt = n_slots / (kAmaxSlots * kAmaxStride);
  check_dev(amax, "amax", at::kFloat, n_slots, 4);
  check_dev(scale, "scale", at::kFloat, nt, 4);
  TORCH_CHECK(hist.size(0) >= nt, "hist rows");
  check_dev(hist, "hist", at::kFloat, nt * hist.size(1), 4);
  check_dev(inv_scale, "inv_scale", at::kFloat, nt, 4);
  check_dev(fmax, "fmax", at::kFloat, nt, 4);
  launch_fp8_update_scale(hist.data_ptr<float>(), (int)hist.size(1), (int)nt, amax.data_ptr<float>(),
                          scale.data_ptr<float>(), inv_scale.data_ptr<float>(), fmax.data_ptr<float>(), margin, step,
                          cur_stream());
}

py::tuple gemm_plan(bool a_mn, bool b_mn, int64_t M, int64_t N, int64_t K, int cfg, int splits, bool accumulate) {
  check_gemm_cfg(cfg);
  const GemmPlan p = plan_gemm_bf16(a_mn, b_mn, (int)M, (int)N, (int)K, cfg, splits, accumulate ? 1 : 0);
  return py::make_tuple(p.cfg, p.splits, p.ksteps, p.ws_floats, p.ext);
}

void colsum(Tensor X, Tensor out, bool accumulate) {
  TORCH_CHECK(X.dim() == 2 && X.scalar_type() == at::kBFloat16 && X.stride(1) == 1 && X.is_cuda(), "colsum X");
  TORCH_CHECK(X.size(1) % 8 == 0 && X.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(X.data_ptr()) % 16 == 0,
              "colsum needs 16-byte aligned rows (columns and row stride multiples of 8)");
  TORCH_CHECK(X.size(0) < (1LL << 31) && X.size(1) < (1LL << 31), "colsum dims too large");
  check_dev(out, "out", at::kFloat, X.size(1), 16);
  const int M = (int)X.size(0), N = (int)X.size(1);
  Tensor ws = at::empty({std::max<int64_t>(colsum_ws_floats(M, N), 4)}, X.options().dtype(at::kFloat));
  launch_colsum_bf16(bf16_ptr(X), M, N, X.stride(0), out.data_ptr<float>(), accumulate ? 1 : 0,
                     ws.data_ptr<float>(), cur_stream());
}

// ----------------------------------------------------------------------------
// LayerNorm / embeddings / attention
// ----------------------------------------------------------------------------
static void check_bf16_2d(const Tensor& t, const char* name, int64_t rows, int64_t cols) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kBFloat16, name,
              " must be a contiguous bf16 device tensor");
  TORCH_CHECK(t.numel() == rows * cols, name, " has ", t.numel(), " elements, expected ", rows, "x", cols);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

// ---------------------------------------------------------------------------- masked-LM head (mlm.hip)
void vocab_ce(Tensor Z, int64_t V, Tensor labels, Tensor row_loss, Tensor row_lse, Tensor row_hit, bool write_grad,
              int64_t ignore_index) {
  TORCH_CHECK(Z.dim() == 2 && Z.is_cuda() && Z.scalar_type() == at::kBFloat16 && Z.stride(1) == 1,
              "vocab_ce: Z must be a bf16 [R, ldz] device tensor with unit column stride");
  const int64_t R = Z.size(0), ldz = Z.size(1);
  TORCH_CHECK(R == 0 || Z.stride(0) == ldz, "vocab_ce: Z rows must be contiguous (the row stride is the padded width)");
  TORCH_CHECK(ldz % 8 == 0 && reinterpret_cast<uintptr_t>(Z.data_ptr()) % 16 == 0,
              "vocab_ce needs ldz % 8 == 0 and a 16-byte aligned base");
  TORCH_CHECK(V >= 1 && V <= ldz && ldz < (1LL << 31), "vocab_ce: 1 <= V <= ldz < 2^31");
  TORCH_CHECK(R < (1LL << 31), "vocab_ce: too many rows");
  check_dev(labels, "labels", at::kLong, R, 8);
  check_dev(row_loss, "row_loss", at::kFloat, R, 4);
  check_dev(row_lse, "row_lse", at::kFloat, R, 4);
  check_dev(row_hit, "row_hit", at::kFloat, R, 4);
  launch_vocab_ce((uint16_t*)Z.data_ptr(), R, ldz, (int)V, labels.data_ptr<int64_t>(), row_loss.data_ptr<float>(),
                  row_lse.data_ptr<float>(), row_hit.data_ptr<float>(), ignore_index, write_grad, cur_stream());
}

void mlm_select(Tensor labels, int64_t P, Tensor slot_row, Tensor slot_label, Tensor seq_overflow, Tensor overflow,
                c10::optional<Tensor> lens, c10::optional<Tensor> cu_seqlens, int64_t ignore_index) {
  TORCH_CHECK(labels.dim() == 2, "mlm_select: labels must be [B, S]");
  const int64_t B = labels.size(0), S = labels.size(1), R = slot_row.numel();
  TORCH_CHECK(P >= 1 && B >= 1 && S >= 1 && B * S < (1LL << 31) && B * P <= R && R < (1LL << 31),
              "mlm_select: need P >= 1, B * S < 2^31 and B * P <= R slots");
  check_dev(labels, "labels", at::kLong, B * S, 8);
  check_dev(slot_row, "slot_row", at::kInt, R, 4);
  check_dev(slot_label, "slot_label", at::kLong, R, 8);
  TORCH_CHECK(slot_label.numel() == R, "mlm_select: slot_label must have as many entries as slot_row");
  check_dev(seq_overflow, "seq_overflow", at::kInt, B, 4);
  check_dev(overflow, "overflow", at::kInt, 1, 4);
  TORCH_CHECK(!(lens.has_value() && cu_seqlens.has_value()), "mlm_select takes lens or cu_seqlens, not both");
  const int* lp = nullptr;
  const int* cp = nullptr;
  if (lens.has_value()) {
    check_dev(*lens, "lens", at::kInt, B, 4);
    lp = lens->data_ptr<int>();
  }
  if (cu_seqlens.has_value()) {
    check_dev(*cu_seqlens, "cu_seqlens", at::kInt, B + 1, 4);
    cp = cu_seqlens->data_ptr<int>();
  }
  launch_mlm_select(labels.data_ptr<int64_t>(), (int)B, (int)S, (int)P, R, lp, cp, ignore_index,
                    slot_row.data_ptr<int>(), slot_label.data_ptr<int64_t>(), seq_overflow.data_ptr<int>(),
                    overflow.data_ptr<int>(), cur_stream());
}

void gather_rows(Tensor X, Tensor slot_row, Tensor out) {
  TORCH_CHECK(X.dim() == 2 && out.dim() == 2 && X.size(1) == out.size(1) && X.size(1) % 8 == 0,
              "gather_rows: X [N, h], out [R, h], h % 8 == 0");
  const int64_t N = X.size(0), h = X.size(1), R = out.size(0);
  TORCH_CHECK(N < (1LL << 31) && R < (1LL << 31), "gather_rows: too many rows");
  check_bf16_2d(X, "X", N, h);
  check_bf16_2d(out, "out", R, h);
  check_dev(slot_row, "slot_row", at::kInt, R, 4);
  launch_gather_rows(bf16_ptr(X), N, (int)h, slot_row.data_ptr<int>(), R, (uint16_t*)out.data_ptr(), cur_stream());
}

void scatter_rows(Tensor G, Tensor slot_row, Tensor dX) {
  TORCH_CHECK(G.dim() == 2 && dX.dim() == 2 && G.size(1) == dX.size(1) && G.size(1) % 8 == 0,
              "scatter_rows: G [R, h], dX [N, h], h % 8 == 0");
  const int64_t R = G.size(0), h = G.size(1), N = dX.size(0);
  TORCH_CHECK(N < (1LL << 31) && R < (1LL << 31), "scatter_rows: too many rows");
  check_bf16_2d(G, "G", R, h);
  check_bf16_2d(dX, "dX", N, h);
  check_dev(slot_row, "slot_row", at::kInt, R, 4);
  launch_scatter_rows(bf16_ptr(G), R, (int)h, slot_row.data_ptr<int>(), N, (uint16_t*)dX.data_ptr(), cur_stream());
}

void ln_fwd(Tensor X, Tensor gamma, Tensor beta, Tensor Y, Tensor mean, Tensor rstd, double eps) {
  const int64_t D = gamma.numel(), rows = X.numel() / std::max<int64_t>(D, 1);
  TORCH_CHECK(D % 256 == 0 && D >= 256 && D <= 1024, "LayerNorm width must be 256/512/768/1024");
  check_bf16_2d(X, "X", rows, D);
  check_bf16_2d(Y, "Y", rows, D);
  check_dev(gamma, "gamma", at::kFloat, D);
  check_dev(beta, "beta", at::kFloat, D);
  check_dev(mean, "mean", at::kFloat, rows, 4);
  check_dev(rstd, "rstd", at::kFloat, rows, 4);
  launch_ln_fwd(bf16_ptr(X), gamma.data_ptr<float>(), beta.data_ptr<float>(), (uint16_t*)Y.data_ptr(),
                mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, (int)D, (float)eps, cur_stream());
}

// One dropout site's kernel arguments: thr = min(int(p * 2^32), 0xFFFFFFFF) (keep iff word >= thr),
// scale = 1 / (1 - p) in double rounded once to fp32 -- the values ops/dropout.py computes.
static DropArgs make_drop_args(double p, int64_t seed, int64_t site, int64_t rank) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout probability must satisfy 0 <= p < 1, got ", p);
  TORCH_CHECK(site >= 0 && site <= 0xFFFFFFFFLL && rank >= 0 && rank <= 0xFFFFFFFFLL,
              "dropout site / rank must fit 32 bits");
  const double t = p * 4294967296.0;
  DropArgs d;
  d.thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  d.scale = (float)(1.0 / (1.0 - p));
  d.seed_lo = (uint32_t)((uint64_t)seed & 0xFFFFFFFFull);
  d.seed_hi = (uint32_t)((uint64_t)seed >> 32);
  d.site = (uint32_t)site;
  d.rank = (uint32_t)rank;
  return d;
}

// The attention-probability site's kernel arguments (one byte per element, mlt_philox.h): thr8 =
// round(p * 256), scale = 1 / (1 - thr8 / 256) in double rounded once to fp32, T = ceil(S / 4) -- the
// values ops/dropout.py computes. p == 0 gives thr8 == 0: the plain kernels run.
static AttnDropArgs make_attn_drop_args(double p, int64_t seed, int64_t site, int64_t rank, int64_t S) {
  TORCH_CHECK_VALUE(p >= 0.0 && p < 1.0, "attention dropout probability must satisfy 0 <= p < 1, got ", p);
  TORCH_CHECK(site >= 0 && site <= 0xFFFFFFFFLL && rank >= 0 && rank <= 0xFFFFFFFFLL,
              "dropout site / rank must fit 32 bits");
  AttnDropArgs d;
  d.thr8 = (uint32_t)std::floor(p * 256.0 + 0.5);
  TORCH_CHECK_VALUE(p == 0.0 || d.thr8 > 0, "attention dropout probability ", p,
                    " rounds to 0/256: no element would be dropped (the smallest effective p is 1/256)");
  TORCH_CHECK_VALUE(d.thr8 < 256, "attention dropout probability ", p, " rounds to 256/256: every element dropped");
  d.scale = (float)(1.0 / (1.0 - (double)d.thr8 / 256.0));
  d.seed_lo = (uint32_t)((uint64_t)seed & 0xFFFFFFFFull);
  d.seed_hi = (uint32_t)((uint64_t)seed >> 32);
  d.site = (uint32_t)site;
  d.rank = (uint32_t)rank;
  d.T = (uint32_t)((S + 3) / 4);
  return d;
}

// out = keep ? bf16(x * scale) : 0 over a contiguous bf16 tensor (flat element index = mask index)
void dropout(Tensor x, Tensor out, double p, int64_t seed, int64_t site, int64_t rank) {
  TORCH_CHECK(x.numel() % 8 == 0, "dropout needs numel % 8 == 0, got ", x.numel());
  check_dev(x, "x", at::kBFloat16, 0, 16);
  check_dev(out, "out", at::kBFloat16, x.numel(), 16);
  TORCH_CHECK(out.numel() == x.numel(), "dropout: out must have x's size");
  launch_dropout(bf16_ptr(x), (uint16_t*)out.data_ptr(), x.numel(), make_drop_args(p, seed, site, rank),
                 cur_stream());
}

// Z = bf16(dropout(Y0) + RES); Y, mean, rstd = LayerNorm(Z)
void dropout_add_ln_fwd(Tensor Y0, Tensor RES, Tensor gamma, Tensor beta, Tensor Z, Tensor Y, Tensor mean,
                        Tensor rstd, double eps, double p, int64_t seed, int64_t site, int64_t rank) {
  const int64_t D = gamma.numel(), rows = Y0.numel() / std::max<int64_t>(D, 1);
  TORCH_CHECK(D % 256 == 0 && D >= 256 && D <= 1024, "LayerNorm width must be 256/512/768/1024");
  check_bf16_2d(Y0, "Y0", rows, D);
  check_bf16_2d(RES, "RES", rows, D);
  check_bf16_2d(Z, "Z", rows, D);
  check_bf16_2d(Y, "Y", rows, D);
  check_dev(gamma, "gamma", at::kFloat, D);
  check_dev(beta, "beta", at::kFloat, D);
  check_dev(mean, "mean", at::kFloat, rows, 4);
  check_dev(rstd, "rstd", at::kFloat, rows, 4);
  launch_dropout_add_ln_fwd(bf16_ptr(Y0), bf16_ptr(RES), gamma.data_ptr<float>(), beta.data_ptr<float>(),
                            (uint16_t*)Z.data_ptr(), (uint16_t*)Y.data_ptr(), mean.data_ptr<float>(),
                            rstd.data_ptr<float>(), rows, (int)D, (float)eps, make_drop_args(p, seed, site, rank),
                            cur_stream());
}

int64_t ln_partial_blocks(int64_t rows) { return ln_bwd_partial_blocks(rows); }

// dxsum (optional): column sums of DX (bias gradient of the producing linear layer), accumulated
// into when dxsum_acc. dxm (optional, needs dxsum, excludes dres): X was dropout(linear) + residual
// at site (p, seed, site, rank); dxm gets mask * scale * DX and dxsum its column sums instead of DX's.
void ln_bwd(Tensor DY, Tensor X, Tensor gamma, Tensor mean, Tensor rstd, Tensor DX, Tensor part, Tensor dgamma,
            Tensor dbeta, bool accumulate, c10::optional<Tensor> dres, c10::optional<Tensor> dxsum,
            bool dxsum_acc, c10::optional<Tensor> dxm, double p, int64_t seed, int64_t site, int64_t rank) {
  const int64_t D = gamma.numel(), rows = X.numel() / std::max<int64_t>(D, 1);
  TORCH_CHECK(D % 256 == 0 && D >= 256 && D <= 1024, "LayerNorm width must be 256/512/768/1024");
  check_bf16_2d(X, "X", rows, D);
  check_bf16_2d(DY, "DY", rows, D);
  check_bf16_2d(DX, "DX", rows, D);
  check_dev(gamma, "gamma", at::kFloat, D);
  check_dev(mean, "mean", at::kFloat, rows, 4);
  check_dev(rstd, "rstd", at::kFloat, rows, 4);
  check_dev(part, "part", at::kFloat, (int64_t)ln_bwd_partial_blocks(rows) * (dxsum.has_value() ? 3 : 2) * D);
  check_dev(dgamma, "dgamma", at::kFloat, D);
  check_dev(dbeta, "dbeta", at::kFloat, D);
  float* dxs = nullptr;
  if (dxsum.has_value()) {
    check_dev(*dxsum, "dxsum", at::kFloat, D);
    dxs = dxsum->data_ptr<float>();
  }
  const uint16_t* dr = nullptr;
  if (dres.has_value()) {
    check_bf16_2d(*dres, "dres", rows, D);
    dr = bf16_ptr(*dres);
  }
  if (dxm.has_value()) {
    TORCH_CHECK(dxs != nullptr && dr == nullptr, "ln_bwd: dxm needs dxsum and takes no dres");
    check_bf16_2d(*dxm, "dxm", rows, D);
    launch_ln_bwd_dropout(bf16_ptr(DY), bf16_ptr(X), gamma.data_ptr<float>(), mean.data_ptr<float>(),
                          rstd.data_ptr<float>(), (uint16_t*)DX.data_ptr(), (uint16_t*)dxm->data_ptr(),
                          part.data_ptr<float>(), dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), rows, (int)D,
                          accumulate ? 1 : 0, dxs, dxsum_acc ? 1 : 0, make_drop_args(p, seed, site, rank),
                          cur_stream());
    return;
  }
  launch_ln_bwd(bf16_ptr(DY), bf16_ptr(X), gamma.data_ptr<float>(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
                (uint16_t*)DX.data_ptr(), part.data_ptr<float>(), dgamma.data_ptr<float>(), dbeta.data_ptr<float>(),
                rows, (int)D, accumulate ? 1 : 0, dr, dxs, dxsum_acc ? 1 : 0, cur_stream());
}

// The dropout form of ln_bwd WITH a residual gradient (pre-norm blocks; ln_bwd itself keeps rejecting the pair):
// DX = rstd (...) + dres, the total gradient of the residual stream, dxm = mask * scale * DX (the dY of the
// linear whose dropped output joined the stream) and dxsum = dxm's column sums. All three are required.
void ln_bwd_dropout_res(Tensor DY, Tensor X, Tensor gamma, Tensor mean, Tensor rstd, Tensor DX, Tensor part,
                        Tensor dgamma, Tensor dbeta, bool accumulate, Tensor dres, Tensor dxsum, bool dxsum_acc,
                        Tensor dxm, double p, int64_t seed, int64_t site, int64_t rank) {
  const int64_t D = gamma.numel(), rows = X.numel() / std::max<int64_t>(D, 1);
  TORCH_CHECK(D % 256 == 0 && D >= 256 && D <= 1024, "LayerNorm width must be 256/512/768/1024");
  check_bf16_2d(X, "X", rows, D);
  check_bf16_2d(DY, "DY", rows, D);
  check_bf16_2d(DX, "DX", rows, D);
  check_bf16_2d(dres, "dres", rows, D);
  check_bf16_2d(dxm, "dxm", rows, D);
  check_dev(gamma, "gamma", at::kFloat, D);
  check_dev(mean, "mean", at::kFloat, rows, 4);
  check_dev(rstd, "rstd", at::kFloat, rows, 4);
  check_dev(part, "part", at::kFloat, (int64_t)ln_bwd_partial_blocks(rows) * 3 * D);
  check_dev(dgamma, "dgamma", at::kFloat, D);
  check_dev(dbeta, "dbeta", at::kFloat, D);
  check_dev(dxsum, "dxsum", at::kFloat, D);
  launch_ln_bwd_dropout_res(bf16_ptr(DY), bf16_ptr(X), gamma.data_ptr<float>(), mean.data_ptr<float>(),
                            rstd.data_ptr<float>(), (uint16_t*)DX.data_ptr(), (uint16_t*)dxm.data_ptr(),
                            part.data_ptr<float>(), dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), rows, (int)D,
                            accumulate ? 1 : 0, bf16_ptr(dres), dxsum.data_ptr<float>(), dxsum_acc ? 1 : 0,
                            make_drop_args(p, seed, site, rank), cur_stream());
}

// RMSNorm: Y = bf16(X rstd gamma), rstd = rsqrt(mean(X^2) + eps)
void rms_fwd(Tensor X, Tensor gamma, Tensor Y, Tensor rstd, double eps) {
  const int64_t D = gamma.numel(), rows = X.numel() / std::max<int64_t>(D, 1);
  TORCH_CHECK(D % 256 == 0 && D >= 256 && D <= 1024, "RMSNorm width must be 256/512/768/1024");
  check_bf16_2d(X, "X", rows, D);
  check_bf16_2d(Y, "Y", rows, D);
  check_dev(gamma, "gamma", at::kFloat, D);
  check_dev(rstd, "rstd", at::kFloat, rows, 4);
  launch_rms_fwd(bf16_ptr(X), gamma.data_ptr<float>(), (uint16_t*)Y.data_ptr(), rstd.data_ptr<float>(), rows, (int)D,
                 (float)eps, cur_stream());
}

// Z = bf16(dropout(Y0) + RES); Y, rstd = RMSNorm(Z)
void dropout_add_rms_fwd(Tensor Y0, Tensor RES, Tensor gamma, Tensor Z, Tensor Y, Tensor rstd, double eps, double p,
                         int64_t seed, int64_t site, int64_t rank) {
  const int64_t D = gamma.numel(), rows = Y0.numel() / std::max<int64_t>(D, 1);
  TORCH_CHECK(D % 256 == 0 && D >= 256 && D <= 1024, "RMSNorm width must be 256/512/768/1024");
  check_bf16_2d(Y0, "Y0", rows, D);
  check_bf16_2d(RES, "RES", rows, D);
  check_bf16_2d(Z, "Z", rows, D);
  check_bf16_2d(Y, "Y", rows, D);
  check_dev(gamma, "gamma", at::kFloat, D);
  check_dev(rstd, "rstd", at::kFloat, rows, 4);
  launch_dropout_add_rms_fwd(bf16_ptr(Y0), bf16_ptr(RES), gamma.data_ptr<float>(), (uint16_t*)Z.data_ptr(),
                             (uint16_t*)Y.data_ptr(), rstd.data_ptr<float>(), rows, (int)D, (float)eps,
                             make_drop_args(p, seed, site, rank), cur_stream());
}

// dxsum (optional): column sums of DX, accumulated into when dxsum_acc. dxm (optional, needs dxsum): X was
// dropout(linear) + residual at site (p, seed, site, rank); dxm gets mask * scale * DX and dxsum its column
// sums instead of DX's. dres (optional, in every form): added into DX. part: ln_partial_blocks(rows) *
// (dxsum ? 2 : 1) * D floats.
void rms_bwd(Tensor DY, Tensor X, Tensor gamma, Tensor rstd, Tensor DX, Tensor part, Tensor dgamma, bool accumulate,
             c10::optional<Tensor> dres, c10::optional<Tensor> dxsum, bool dxsum_acc, c10::optional<Tensor> dxm,
             double p, int64_t seed, int64_t site, int64_t rank) {
  const int64_t D = gamma.numel(), rows = X.numel() / std::max<int64_t>(D, 1);
  TORCH_CHECK(D % 256 == 0 && D >= 256 && D <= 1024, "RMSNorm width must be 256/512/768/1024");
  check_bf16_2d(X, "X", rows, D);
  check_bf16_2d(DY, "DY", rows, D);
  check_bf16_2d(DX, "DX", rows, D);
  check_dev(gamma, "gamma", at::kFloat, D);
  check_dev(rstd, "rstd", at::kFloat, rows, 4);
  check_dev(part, "part", at::kFloat, (int64_t)ln_bwd_partial_blocks(rows) * (dxsum.has_value() ? 2 : 1) * D);
  check_dev(dgamma, "dgamma", at::kFloat, D);
  float* dxs = nullptr;
  if (dxsum.has_value()) {
    check_dev(*dxsum, "dxsum", at::kFloat, D);
    dxs = dxsum->data_ptr<float>();
  }
  const uint16_t* dr = nullptr;
  if (dres.has_value()) {
    check_bf16_2d(*dres, "dres", rows, D);
    dr = bf16_ptr(*dres);
  }
  uint16_t* dm = nullptr;
  DropArgs da{};
  if (dxm.has_value()) {
    TORCH_CHECK(dxs != nullptr, "rms_bwd: dxm needs dxsum");
    check_bf16_2d(*dxm, "dxm", rows, D);
    dm = (uint16_t*)dxm->data_ptr();
    da = make_drop_args(p, seed, site, rank);
  }
  launch_rms_bwd(bf16_ptr(DY), bf16_ptr(X), gamma.data_ptr<float>(), rstd.data_ptr<float>(), (uint16_t*)DX.data_ptr(),
                 dm, part.data_ptr<float>(), dgamma.data_ptr<float>(), rows, (int)D, accumulate ? 1 : 0, dr, dxs,
                 dxsum_acc ? 1 : 0, da, cur_stream());
}

// pos (packed batches): int32 [rows], the position of every token inside its own sequence (< S);
// without it the batch is padded [B, S] and pos = row % S
// Wp None (rotary positions): no position table, out = word + type
void embed_fwd(Tensor ids, c10::optional<Tensor> tt, Tensor Ww, c10::optional<Tensor> Wp, Tensor Wt, Tensor out,
               int64_t S, c10::optional<Tensor> pos) {
  const int64_t rows = ids.numel(), D = Ww.size(1);
  TORCH_CHECK(D % 256 == 0 && D <= 1024, "embedding width must be a multiple of 256 (<= 1024)");
  TORCH_CHECK(S > 0 && (!Wp.has_value() || S <= Wp->size(0)), "sequence length vs position table");
  const int* pp = nullptr;
  if (pos.has_value()) {
    check_dev(*pos, "pos", at::kInt, rows, 4);
    TORCH_CHECK(pos->numel() == rows, "embed_fwd: pos must have one entry per token");
    pp = pos->data_ptr<int>();
  } else {
    TORCH_CHECK(rows % S == 0, "sequence length vs token count (padded batches are [B, S])");
  }
  check_dev(ids, "ids", at::kLong, rows, 8);
  const int64_t* tp = nullptr;
  if (tt.has_value()) {
    check_dev(*tt, "token_type", at::kLong, rows, 8);
    tp = tt->data_ptr<int64_t>();
  }
  check_bf16_2d(Ww, "word_emb", Ww.size(0), D);
  if (Wp.has_value()) check_bf16_2d(*Wp, "pos_emb", Wp->size(0), D);
  check_bf16_2d(Wt, "type_emb", Wt.size(0), D);
  TORCH_CHECK(Wt.size(0) <= 2, "at most 2 token types");
  check_bf16_2d(out, "out", rows, D);
  launch_embed_fwd(ids.data_ptr<int64_t>(), tp, bf16_ptr(Ww), Wp.has_value() ? bf16_ptr(*Wp) : nullptr, bf16_ptr(Wt),
                   (uint16_t*)out.data_ptr(), rows, (int)S, (int)D, Ww.size(0), (int)Wt.size(0), cur_stream(), pp);
}

// cu_seqlens (packed batches): int32 [B + 1] on the device, sequence b = rows cu[b] .. cu[b + 1] (each at
// most S long, cu[B] <= rows); without it the batch is padded [B, S]
// gp None (rotary positions): no position table, no position gradient is written
void embed_bwd(Tensor sid, Tensor perm, c10::optional<Tensor> tt, Tensor DX, Tensor gw, c10::optional<Tensor> gp,
               Tensor gt, Tensor part, int64_t S, c10::optional<Tensor> cu_seqlens) {
  const int64_t rows = sid.numel(), D = gw.size(1);
  TORCH_CHECK(D % 256 == 0 && D <= 1024, "embedding width");
  TORCH_CHECK(S > 0 && (!gp.has_value() || S <= gp->size(0)), "sequence length vs position table");
  const int* cu = nullptr;
  int64_t Bc = 0;
  if (cu_seqlens.has_value()) {
    check_dev(*cu_seqlens, "cu_seqlens", at::kInt, 2, 4);
    Bc = cu_seqlens->numel() - 1;
    TORCH_CHECK(rows <= Bc * S && Bc <= 0x7fffffff, "embed_bwd: ", rows, " packed rows exceed B * S = ", Bc * S);
    cu = cu_seqlens->data_ptr<int>();
  } else {
    TORCH_CHECK(rows % S == 0, "sequence length vs token count (padded batches are [B, S])");
  }
  check_dev(sid, "sorted ids", at::kLong, rows, 8);
  check_dev(perm, "perm", at::kLong, rows, 8);
  const int64_t* tp = nullptr;
  if (tt.has_value()) {
    check_dev(*tt, "token_type", at::kLong, rows, 8);
    tp = tt->data_ptr<int64_t>();
  }
  check_bf16_2d(DX, "DX", rows, D);
  check_dev(gw, "gw", at::kFloat, gw.size(0) * D, 16);
  if (gp.has_value()) check_dev(*gp, "gp", at::kFloat, gp->size(0) * D, 16);
  check_dev(gt, "gt", at::kFloat, gt.size(0) * D);
  TORCH_CHECK(gt.size(0) <= 2, "at most 2 token types");
  check_dev(part, "part", at::kFloat, S * 2 * D, 16);
  launch_embed_bwd(sid.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), tp, bf16_ptr(DX), gw.data_ptr<float>(),
                   gp.has_value() ? gp->data_ptr<float>() : nullptr, gt.data_ptr<float>(), part.data_ptr<float>(), rows,
                   (int)S, (int)D, gw.size(0), (int)gt.size(0), cur_stream(), cu, (int)Bc);
}

// Rotary position embedding of the q and k columns of qkv [rows, 3 * H * 64] in place (rope.hip). qkv may be a
// row-strided view (as attn_decode's qkv_new). table fp32 [P, 32, 2]. The position of a row is pos[row] (int32
// [rows] on the device; clamped into the table in the kernel, checked there in debug builds) or, without pos,
// row % S with S <= P. sign = +1: the rotation, -1: the inverse rotation (the backward, on dQKV).
void rope_qk(Tensor qkv, Tensor table, int64_t H, int64_t S, c10::optional<Tensor> pos, int64_t sign) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dim() == 2 && qkv.scalar_type() == at::kBFloat16,
              "rope_qk: qkv must be a bf16 [rows, 3 * H * 64] device tensor");
  const int64_t rows = qkv.size(0), D = H * 64;
  TORCH_CHECK(H > 0 && H <= 65535, "rope_qk: heads");
  TORCH_CHECK(qkv.size(1) == 3 * D, "rope_qk: qkv has ", qkv.size(1), " columns, expected 3 * H * 64 = ", 3 * D);
  TORCH_CHECK(sign == 1 || sign == -1, "rope_qk: sign must be +1 or -1, got ", sign);
  check_dev(table, "rope table", at::kFloat, 64, 16);
  TORCH_CHECK(table.dim() == 3 && table.size(1) == 32 && table.size(2) == 2, "rope_qk: table must be [P, 32, 2]");
  const int64_t P = table.size(0);
  TORCH_CHECK(P <= 0x7fffffff, "rope_qk: table rows");
  if (rows == 0) return;
  TORCH_CHECK(qkv.stride(1) == 1 && qkv.stride(0) >= 3 * D && qkv.stride(0) % 8 == 0,
              "rope_qk: qkv needs unit column stride and a row stride that is a multiple of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, "rope_qk: qkv must be 16-byte aligned");
  TORCH_CHECK(rows * H * 8 <= 0x7fffffff, "rope_qk: ", rows, " rows x ", H, " heads exceed the kernel's index range");
  const int* pp = nullptr;
  if (pos.has_value()) {
    check_dev(*pos, "pos", at::kInt, rows, 4);
    TORCH_CHECK(pos->numel() == rows, "rope_qk: pos must have one entry per row");
    pp = pos->data_ptr<int>();
    S = 1;
  } else {
    TORCH_CHECK(S > 0 && S <= P, "rope_qk: sequence length ", S, " vs a table of ", P, " positions");
  }
  launch_rope_qk((uint16_t*)qkv.data_ptr(), qkv.stride(0), rows, (int)H, table.data_ptr<float>(), (int)P, (int)S, pp,
                 (int)sign, cur_stream());
}

static const int* lens_ptr(const c10::optional<Tensor>& lens, int64_t B) {
  if (!lens.has_value()) return nullptr;
  check_dev(*lens, "lens", at::kInt, B, 4);
  return lens->data_ptr<int>();
}

// Packed batches: cu_seqlens int32 [B + 1] on the device; returns the token-row count T the tensors must
// agree on (qkv.numel() / 3D, at most B * S), or B * S for a padded batch. cu[B] <= T (rows past cu[B]
// belong to no sequence and stay untouched) cannot be checked here without a device read: debug builds
// check it in the kernels (MLT_DCHECK).
static int64_t attn_rows(const c10::optional<Tensor>& cu, const Tensor& qkv, int64_t B, int64_t S, int64_t D,
                         const int** cup) {
  *cup = nullptr;
  if (!cu.has_value()) return B * S;
  check_dev(*cu, "cu_seqlens", at::kInt, B + 1, 4);
  TORCH_CHECK(cu->numel() == B + 1, "cu_seqlens has ", cu->numel(), " elements, expected B + 1 = ", B + 1);
  TORCH_CHECK(D > 0 && qkv.numel() % (3 * D) == 0, "qkv must be [T, 3 * H * 64]");
  const int64_t T = qkv.numel() / (3 * D);
  TORCH_CHECK(T <= B * S && T <= 0x7fffffff, "packed attention: ", T, " token rows exceed B * S = ", B * S);
  *cup = cu->data_ptr<int>();
  return T;
}

// p, seed, site, rank: attention-probability dropout inside the kernel (p == 0: none)
// cu_seqlens: packed (unpadded) batch, see attn_rows; S is then max_seqlen and lens is unused
void attn_fwd(Tensor qkv, Tensor out, Tensor lse, c10::optional<Tensor> lens, int64_t B, int64_t S, int64_t H,
              double scale, double p, int64_t seed, int64_t site, int64_t rank, c10::optional<Tensor> cu_seqlens,
              bool causal) {
  const int64_t D = H * 64;
  TORCH_CHECK(B > 0 && S > 0 && H > 0 && B <= 65535 && H <= 65535, "attention dims");
  const int* cu = nullptr;
  const int64_t T = attn_rows(cu_seqlens, qkv, B, S, D, &cu);
  check_bf16_2d(qkv, "qkv", T, 3 * D);
  check_bf16_2d(out, "out", T, D);
  check_dev(lse, "lse", at::kFloat, B * H * S, 4);
  const AttnDropArgs ad = make_attn_drop_args(p, seed, site, rank, S);
  const int* lp = cu ? nullptr : lens_ptr(lens, B);
  const AttnProblem prob{(int)B, (int)S, (int)H, (float)scale, lp, cu, (int)T, causal, ad};
  launch_attn_fwd(prob, bf16_ptr(qkv), (uint16_t*)out.data_ptr(), lse.data_ptr<float>(), cur_stream());
}

// Single-token attention over one layer's cache kv [2, B, H, Smax, 64], the append of the new token fused in
// (attn_decode.hip). qkv_new [B, 3 * H * 64] may be a row-strided view. pos int32 [B] stays on the device:
// pos[b] < Smax cannot be checked here without a read (debug builds check it in the kernel, MLT_DCHECK).
// rope (fp32 [P >= Smax, 32, 2], the table of ops/rope.py): the ROPE instantiation, q and the new k rotated by
// pos[b] and rounded to bf16 before use; None: the kernel without rotation.
void attn_decode(Tensor qkv_new, Tensor kv, Tensor pos, Tensor out, int64_t H, double scale,
                 c10::optional<Tensor> rope) {
  TORCH_CHECK(qkv_new.is_cuda() && qkv_new.dim() == 2 && qkv_new.scalar_type() == at::kBFloat16,
              "attn_decode: qkv_new must be a bf16 [B, 3 * H * 64] device tensor");
  const int64_t B = qkv_new.size(0), D = H * 64;
  TORCH_CHECK(B > 0 && H > 0 && B <= 65535 && H <= 65535, "attention dims");
  TORCH_CHECK(qkv_new.size(1) == 3 * D, "attn_decode: qkv_new has ", qkv_new.size(1), " columns, expected 3 * H * 64 = ",
              3 * D);
  TORCH_CHECK(qkv_new.stride(1) == 1 && qkv_new.stride(0) >= 3 * D && qkv_new.stride(0) % 8 == 0,
              "attn_decode: qkv_new needs unit column stride and a row stride that is a multiple of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv_new.data_ptr()) % 16 == 0, "qkv_new must be 16-byte aligned");
  check_dev(kv, "kv", at::kBFloat16, 0);
  TORCH_CHECK(kv.dim() == 5 && kv.size(0) == 2 && kv.size(1) == B && kv.size(2) == H && kv.size(3) >= 1 &&
                  kv.size(4) == 64,
              "attn_decode: kv must be [2, B, H, Smax, 64] = [2, ", B, ", ", H, ", Smax, 64]");
  const int64_t Smax = kv.size(3);
  TORCH_CHECK(kv.numel() == 2 * B * H * Smax * 64 && Smax <= 0x7fffffff, "attn_decode: kv size");
  check_dev(pos, "pos", at::kInt, B, 4);
  TORCH_CHECK(pos.numel() == B, "attn_decode: pos must have one entry per sequence");
  check_bf16_2d(out, "out", B, D);
  const float* rp = nullptr;
  if (rope.has_value()) {
    check_dev(*rope, "rope table", at::kFloat, 64, 16);
    TORCH_CHECK(rope->dim() == 3 && rope->size(1) == 32 && rope->size(2) == 2 && rope->size(0) >= Smax,
                "attn_decode: the rope table must be [P >= Smax = ", Smax, ", 32, 2]");
    rp = rope->data_ptr<float>();
  }
  launch_attn_decode(bf16_ptr(qkv_new), qkv_new.stride(0), (uint16_t*)kv.data_ptr(), pos.data_ptr<int>(),
                     (uint16_t*)out.data_ptr(), (int)B, (int)H, (int)Smax, (float)scale, cur_stream(), rp);
}

// The logits operand of the sampling kernels: fp32 [B, >= V] with unit column stride, a row stride ldz % 4 == 0
// and a 16-byte aligned base (16-byte loads), every row readable up to round_up(V, 4) columns. The [B, V] view
// of the padded [B, Vp] buffer that ops.mlm.decode_logits returns qualifies as it is.
static int64_t check_sample_logits(const Tensor& logits, int64_t V, const char* who) {
  TORCH_CHECK(logits.defined() && logits.is_cuda() && logits.dim() == 2 && logits.scalar_type() == at::kFloat, who,
              ": logits must be an fp32 [B, ldz] device tensor");
  const int64_t B = logits.size(0), ldz = B > 1 ? logits.stride(0) : (V + 3) / 4 * 4;  // one row: no stride
  TORCH_CHECK(B >= 1 && B <= 65535, who, ": 1 <= B <= 65535, got ", B);
  TORCH_CHECK(logits.stride(1) == 1, who, ": logits need unit column stride");
  TORCH_CHECK(ldz % 4 == 0, who, ": the row stride ldz must be a multiple of 4, got ", ldz);
  TORCH_CHECK(V >= 1 && V <= logits.size(1) && V <= ldz && ldz < (1LL << 31), who, ": 1 <= V <= ldz does not hold: V = ", V,
              ", columns = ", logits.size(1), ", ldz = ", ldz);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0, who, ": logits must be 16-byte aligned");
  const int64_t last = logits.storage_offset() + (B - 1) * ldz + (V + 3) / 4 * 4;  // one past the last element read
  TORCH_CHECK(ldz >= (V + 3) / 4 * 4, who, ": rows overlap: ldz = ", ldz, " < round_up(V, 4)");
  TORCH_CHECK(last * 4 <= (int64_t)logits.storage().nbytes(), who, ": the last row is not readable up to round_up(V, 4)");
  return ldz;
}

// One sampling step (sample.hip; the definition is the header of mlt_sample.h). params int32 [8] = SampleParams,
// per-row state on the logits' device. Nothing is allocated, nothing is read back: capturable.
void sample_step(Tensor logits, int64_t V, Tensor params, Tensor draws, Tensor seq_ids, Tensor finished, Tensor lengths,
                 Tensor tokens, Tensor next_ids, Tensor n_kept) {
  const int64_t ldz = check_sample_logits(logits, V, "sample_step");
  const int64_t B = logits.size(0);
  check_dev(params, "params", at::kInt, 8, 16);
  TORCH_CHECK(params.numel() == 8, "sample_step: params must be int32 [8]");
  check_dev(draws, "draws", at::kInt, B, 4);
  check_dev(seq_ids, "seq_ids", at::kInt, B, 4);
  check_dev(finished, "finished", at::kInt, B, 4);
  check_dev(n_kept, "n_kept", at::kInt, B, 4);
  check_dev(lengths, "lengths", at::kLong, B, 8);
  check_dev(next_ids, "next_ids", at::kLong, B, 8);
  check_dev(tokens, "tokens", at::kLong, B, 8);
  TORCH_CHECK(draws.numel() == B && seq_ids.numel() == B && finished.numel() == B && n_kept.numel() == B &&
                  lengths.numel() == B && next_ids.numel() == B,
              "sample_step: draws / seq_ids / finished / n_kept / lengths / next_ids must have B = ", B, " entries");
  TORCH_CHECK(tokens.dim() == 2 && tokens.size(0) == B && tokens.size(1) >= 1 && tokens.size(1) <= 0x7fffffff,
              "sample_step: tokens must be int64 [B, T], T >= 1");
  for (const Tensor* t : {&params, &draws, &seq_ids, &finished, &n_kept, &lengths, &next_ids, &tokens})
    TORCH_CHECK(t->device() == logits.device(), "sample_step: every operand must be on the logits' device");
  launch_sample_step(logits.data_ptr<float>(), ldz, (int)V, (int)B, reinterpret_cast<const SampleParams*>(params.data_ptr<int>()),
                     draws.data_ptr<int>(), seq_ids.data_ptr<int>(), finished.data_ptr<int>(), lengths.data_ptr<int64_t>(),
                     tokens.data_ptr<int64_t>(), (int)tokens.size(1), next_ids.data_ptr<int64_t>(),
                     n_kept.data_ptr<int>(), cur_stream());
}

// Test support: the integer weights of step 2 (int32 [B, V], values in [0, 2^24]) and the argmax (int32 [B]),
// from a plain kernel that calls the inline functions sample_step calls.
std::tuple<Tensor, Tensor> sample_weights(Tensor logits, int64_t V, double inv_t_log2e) {
  const int64_t ldz = check_sample_logits(logits, V, "sample_weights");
  const int64_t B = logits.size(0);
  Tensor w = at::empty({B, V}, logits.options().dtype(at::kInt));
  Tensor a = at::empty({B}, logits.options().dtype(at::kInt));
  launch_sample_weights(logits.data_ptr<float>(), ldz, (int)V, (int)B, (float)inv_t_log2e, w.data_ptr<int>(),
                        a.data_ptr<int>(), cur_stream());
  return {w, a};
}

void attn_bwd(Tensor qkv, Tensor out, Tensor dout, Tensor lse, Tensor delta, c10::optional<Tensor> lens, Tensor dqkv,
              int64_t B, int64_t S, int64_t H, double scale, c10::optional<Tensor> colsum_out,
              bool colsum_accumulate, c10::optional<Tensor> q8_y, c10::optional<Tensor> q8_yt,
              c10::optional<Tensor> q8_scale, c10::optional<Tensor> q8_amax, double p, int64_t seed, int64_t site,
              int64_t rank, c10::optional<Tensor> cu_seqlens, bool causal) {
  const int64_t D = H * 64;
  TORCH_CHECK(B > 0 && S > 0 && H > 0 && B <= 65535 && H <= 65535, "attention dims");
  const AttnDropArgs ad = make_attn_drop_args(p, seed, site, rank, S);  // the forward's (p, seed, site, rank)
  const int* cu = nullptr;
  const int64_t T = attn_rows(cu_seqlens, qkv, B, S, D, &cu);
  const int* lp = cu ? nullptr : lens_ptr(lens, B);
  const AttnProblem prob{(int)B, (int)S, (int)H, (float)scale, lp, cu, (int)T, causal, ad};
  // which kernels run it; a combination without a kernel is refused here, before any other q8 check
  const AttnBwdRoute route = attn_bwd_route(prob, q8_y.has_value());
  check_bf16_2d(qkv, "qkv", T, 3 * D);
  check_bf16_2d(out, "out", T, D);
  check_bf16_2d(dout, "dout", T, D);
  check_bf16_2d(dqkv, "dqkv", T, 3 * D);
  check_dev(lse, "lse", at::kFloat, B * H * S, 4);
  check_dev(delta, "delta", at::kFloat, T * H, 4);
  Tensor pq, pkv;
  if (colsum_out.has_value()) {  // QKV bias gradient = column sums of dQKV, from the backward kernels
    check_dev(*colsum_out, "colsum_out", at::kFloat, 3 * D, 16);
    const int64_t rows = B * ((S + 63) / 64);
    pq = at::empty({rows * D}, qkv.options().dtype(at::kFloat));
    pkv = at::empty({rows * 2 * D}, qkv.options().dtype(at::kFloat));
  }
  AttnQ8 q8;
  if (q8_y.has_value()) {  // fp8 training: e5m2 dQKV + transpose + amax instead of the bf16 dQKV
    TORCH_CHECK(q8_yt.has_value() && q8_scale.has_value() && q8_amax.has_value(), "attn_bwd q8: y, yt, scale, amax");
    TORCH_CHECK(q8_y->scalar_type() == at::kFloat8_e5m2 && q8_yt->scalar_type() == at::kFloat8_e5m2,
                "attn_bwd q8: e5m2 outputs");
    TORCH_CHECK(q8_y->is_cuda() && q8_y->is_contiguous() && q8_y->dim() == 2 && q8_y->size(0) == B * S &&
                    q8_y->size(1) == 3 * D, "attn_bwd q8: y must be [B*S, 3D] contiguous");
    TORCH_CHECK(q8_yt->is_cuda() && q8_yt->is_contiguous() && q8_yt->dim() == 2 && q8_yt->size(0) == 3 * D &&
                    q8_yt->size(1) == B * S, "attn_bwd q8: yt must be [3D, B*S] contiguous");
    TORCH_CHECK(S % 16 == 0 && reinterpret_cast<uintptr_t>(q8_yt->data_ptr()) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(q8_y->data_ptr()) % 4 == 0, "attn_bwd q8: S % 16 == 0, aligned outputs");
    check_dev(*q8_scale, "q8_scale", at::kFloat, 1, 4);
    check_dev(*q8_amax, "q8_amax", at::kFloat, (int64_t)kAmaxSlots * kAmaxStride, 4);
    q8.y = (uint8_t*)q8_y->data_ptr();
    q8.yt = (uint8_t*)q8_yt->data_ptr();
    q8.scale = q8_scale->data_ptr<float>();
    q8.amax = q8_amax->data_ptr<float>();
    q8.ldt = B * S;
  }
  launch_attn_bwd(prob, route, bf16_ptr(qkv), bf16_ptr(out), bf16_ptr(dout), lse.data_ptr<float>(),
                  delta.data_ptr<float>(), (uint16_t*)dqkv.data_ptr(), q8, pq.defined() ? pq.data_ptr<float>() : nullptr,
                  pkv.defined() ? pkv.data_ptr<float>() : nullptr, cur_stream());
  if (!colsum_out.has_value()) return;
  float* cs = colsum_out->data_ptr<float>();
  if (route.ring) {  // the ring kernels left column partials: dQ's into cs[0, D), dK | dV's into cs[D, 3D)
    reduce_col_partials(pq, route.rows_q, D, cs, colsum_accumulate);
    reduce_col_partials(pkv, route.rows_kv, 2 * D, cs + D, colsum_accumulate);
  } else {
    Tensor ws = at::empty({std::max<int64_t>(colsum_ws_floats((int)T, (int)(3 * D)), 4)},
                          qkv.options().dtype(at::kFloat));
    launch_colsum_bf16((const uint16_t*)dqkv.data_ptr(), (int)T, (int)(3 * D), dqkv.stride(0), cs,
                       colsum_accumulate ? 1 : 0, ws.data_ptr<float>(), cur_stream());
  }
}

// ----------------------------------------------------------------------------
// Native RCCL communicator over torch tensors (enqueued on the current stream, so
// collectives order with compute and can be captured into hipGraphs).
// ----------------------------------------------------------------------------
static CommDtype comm_dtype(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return CommDtype::F32;
    case at::kBFloat16: return CommDtype::BF16;
    case at::kHalf: return CommDtype::F16;
    case at::kInt: return CommDtype::I32;
    case at::kLong: return CommDtype::I64;
    case at::kByte: return CommDtype::U8;
    default: TORCH_CHECK(false, "unsupported dtype for a collective: ", t.scalar_type());
  }
}

static CommOp comm_op(const std::string& op) {
  if (op == "sum") return CommOp::SUM;
  if (op == "avg") return CommOp::AVG;
  if (op == "max") return CommOp::MAX;
  if (op == "min") return CommOp::MIN;
  TORCH_CHECK(false, "unknown reduce op ", op);
}

class PyComm {
 public:
  PyComm(py::bytes uid, int nranks, int rank, int device) : c_(std::string(uid), nranks, rank, device) {}
  static py::bytes unique_id() { return py::bytes(Communicator::unique_id()); }
  int rank() const { return c_.rank(); }
  int size() const { return c_.size(); }
  void all_reduce(Tensor t, const std::string& op) {
    chk(t);
    c_.all_reduce(t.data_ptr(), t.data_ptr(), t.numel(), comm_dtype(t), comm_op(op), cur_stream());
  }
  void reduce_scatter(Tensor in, Tensor out, const std::string& op) {
    chk(in);
    chk(out);
    TORCH_CHECK(in.numel() == out.numel() * c_.size() && in.scalar_type() == out.scalar_type(), "reduce_scatter sizes");
    c_.reduce_scatter(in.data_ptr(), out.data_ptr(), out.numel(), comm_dtype(in), comm_op(op), cur_stream());
  }
  void all_gather(Tensor in, Tensor out) {
    chk(in);
    chk(out);
    TORCH_CHECK(out.numel() == in.numel() * c_.size() && in.scalar_type() == out.scalar_type(), "all_gather sizes");
    c_.all_gather(in.data_ptr(), out.data_ptr(), in.numel(), comm_dtype(in), cur_stream());
  }
  void broadcast(Tensor t, int root) {
    chk(t);
    TORCH_CHECK(root >= 0 && root < c_.size(), "broadcast root");
    c_.broadcast(t.data_ptr(), t.data_ptr(), t.numel(), comm_dtype(t), root, cur_stream());
  }
  void all_to_all(Tensor in, Tensor out) {
    chk(in);
    chk(out);
    TORCH_CHECK(in.numel() == out.numel() && in.numel() % c_.size() == 0 && in.scalar_type() == out.scalar_type(),
                "all_to_all sizes");
    c_.all_to_all(in.data_ptr(), out.data_ptr(), in.numel() / c_.size(), comm_dtype(in), cur_stream());
  }
  std::string async_error() const { return c_.async_error(); }
  void abort() { c_.abort(); }
  Communicator& raw() { return c_; }

 private:
  void chk(const Tensor& t) const {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "collective tensors must be contiguous device tensors");
    TORCH_CHECK(t.get_device() == c_.device(), "tensor on device ", t.get_device(), ", communicator on ",
                c_.device());
  }
  Communicator c_;
};

class PyXgmi {
 public:
  PyXgmi(int64_t cap, int world, int rank, int device, int blocks) : x_(cap, world, rank, device, blocks) {}
  py::bytes handle() const { return py::bytes(x_.handle()); }
  void open(const std::vector<py::bytes>& hs) {
    std::vector<std::string> v;
    for (const auto& h : hs) v.push_back(std::string(h));
    x_.open(v);
  }
  void all_reduce(Tensor t, bool average) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat, "xgmi all_reduce: fp32 device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "xgmi all_reduce: 16-byte aligned tensor");
    x_.launch(t.data_ptr<float>(), t.numel(), average ? 1.f / x_.world() : 1.f, cur_stream());
  }
  unsigned error() const { return x_.error(); }
  void set_timeout_ms(long long ms) { x_.set_timeout_ms(ms); }
  long long timeout_ms() const { return x_.timeout_ms(); }
  void set_algo(int a) { x_.set_algo(a); }
  int algo() const { return x_.algo(); }
  void set_fault(int f) { x_.set_fault(f); }
  int fault() const { return x_.fault(); }
  void set_fused_two(bool t) { x_.set_fused_two(t); }
  bool fused_two() const { return x_.fused_two(); }
  XgmiAllReduce& raw() { return x_; }

 private:
  XgmiAllReduce x_;
};

// Pinned-host staging slots exposed as CPU uint8 tensors (collate straight into them).
class PyPrefetcher {
 public:
  PyPrefetcher(int64_t slot_bytes, int depth, int device) : p_((size_t)slot_bytes, depth, device), bytes_(slot_bytes) {}
  Tensor slot(int i) {
    TORCH_CHECK(i >= 0 && i < p_.depth(), "slot index");
    return torch::from_blob(p_.slot_ptr(i), {bytes_}, torch::TensorOptions().dtype(at::kByte));
  }
  void copy_to_device(int i, Tensor dst, int64_t nbytes) {
    TORCH_CHECK(dst.is_cuda() && dst.is_contiguous(), "dst must be a contiguous device tensor");
    TORCH_CHECK(nbytes >= 0 && nbytes <= bytes_ && nbytes <= (int64_t)(dst.numel() * dst.element_size()),
                "copy size");
    TORCH_CHECK(i >= 0 && i < p_.depth(), "slot index");
    p_.copy_to_device(i, dst.data_ptr(), (size_t)nbytes);
  }
  // the current stream waits for slot i's copy (call where the batch is consumed)
  void acquire(int i) {
    TORCH_CHECK(i >= 0 && i < p_.depth(), "slot index");
    p_.acquire(i, cur_stream());
  }
  // the current stream's work on device buffer i is enqueued: its next copy may follow it
  void release(int i) {
    TORCH_CHECK(i >= 0 && i < p_.depth(), "slot index");
    p_.release(i, cur_stream());
  }
  bool ready(int i) {
    TORCH_CHECK(i >= 0 && i < p_.depth(), "slot index");
    return p_.slot_ready(i);
  }
  void wait(int i) {
    TORCH_CHECK(i >= 0 && i < p_.depth(), "slot index");
    p_.wait_slot(i);
  }
  int depth() const { return p_.depth(); }
  int64_t slot_bytes() const { return bytes_; }

 private:
  PinnedPrefetcher p_;
  int64_t bytes_;
};

// ----------------------------------------------------------------------------
// LeNet engine: holds every buffer pointer once, launches the fused step, and
// captures multi-step hipGraphs.
// ----------------------------------------------------------------------------
class LeNetEngine {
 public:
  LeNetEngine(int cfg, int max_batch, py::dict bufs) : cfg_(cfg), max_b_(max_batch) {
    TORCH_CHECK(cfg == LENET_DEFAULT || cfg == LENET_TINY, "unknown LeNet cfg");
    TORCH_CHECK(max_batch > 0 && max_batch <= (1 << 20), "bad max_batch");
    const int C1 = cfg == LENET_TINY ? 4 : 6, C2 = cfg == LENET_TINY ? 8 : 16;
    const int F1 = cfg == LENET_TINY ? 64 : 120, F2 = cfg == LENET_TINY ? 32 : 84, NC = 10;
    const int FLAT = C2 * 25;
    const int64_t B = max_batch;
    auto get = [&](const char* k, at::ScalarType st, int64_t n) -> Tensor {
      TORCH_CHECK(bufs.contains(k), "missing engine buffer ", k);
      Tensor t = bufs[k].cast<Tensor>();
      check_dev(t, k, st, n);
      keep_.push_back(t);
      return t;
    };
    auto fp = [&](const char* k, int64_t n) { return get(k, at::kFloat, n).data_ptr<float>(); };
    P_.w1 = fp("w1", C1 * 75);
    P_.b1 = fp("b1", C1);
    P_.w2 = fp("w2", C2 * C1 * 25);
    P_.b2 = fp("b2", C2);
    P_.w3 = fp("w3", (int64_t)F1 * FLAT);
    P_.b3 = fp("b3", F1);
    P_.w4 = fp("w4", F2 * F1);
    P_.b4 = fp("b4", F2);
    P_.w5 = fp("w5", NC * F2);
    P_.b5 = fp("b5", NC);
    P_.gw1 = fp("gw1", C1 * 75);
    P_.gb1 = fp("gb1", C1);
    P_.gw2 = fp("gw2", C2 * C1 * 25);
    P_.gb2 = fp("gb2", C2);
    P_.gw3 = fp("gw3", (int64_t)F1 * FLAT);
    P_.gb3 = fp("gb3", F1);
    P_.gw4 = fp("gw4", F2 * F1);
    P_.gb4 = fp("gb4", F2);
    P_.gw5 = fp("gw5", NC * F2);
    P_.gb5 = fp("gb5", NC);
    P_.x = fp("x", B * 3072);
    P_.p1 = fp("p1", B * C1 * 196);
    P_.p2 = fp("p2", B * FLAT);
    P_.h1 = fp("h1", B * F1);
    P_.h2 = fp("h2", B * F2);
    P_.logits = fp("logits", B * NC);
    P_.dlogits = fp("dlogits", B * NC);
    P_.dh2 = fp("dh2", B * F2);
    P_.dh1 = fp("dh1", B * F1);
    P_.dflat = fp("dflat", B * FLAT);
    P_.g1 = fp("g1", B * C1 * 196);
    P_.slab1 = fp("slab1", B * C1 * 640);  // kSlabStride floats per (sample, channel)
    P_.i1 = get("i1", at::kByte, B * C1 * 196).data_ptr<uint8_t>();
    P_.i2 = get("i2", at::kByte, B * FLAT).data_ptr<uint8_t>();
    P_.targets = get("targets", at::kLong, B).data_ptr<int64_t>();
    P_.stats = get("stats", at::kDouble, 2).data_ptr<double>();  // 16B-aligned by get()
    P_.counters = reinterpret_cast<unsigned*>(get("counters", at::kInt, C1 + 1).data_ptr<int32_t>());
    P_.stage = bufs.contains("stage") ? get("stage", at::kByte, B * 3072).data_ptr<uint8_t>() : nullptr;
    P_.stage_meta = bufs.contains("stage_meta") ? get("stage_meta", at::kLong, B * 4).data_ptr<int64_t>() : nullptr;
    if (!P_.stage || !P_.stage_meta) P_.stage = nullptr, P_.stage_meta = nullptr;
    P_.cestat = bufs.contains("cestat") ? get("cestat", at::kDouble, B * 2).data_ptr<double>() : nullptr;
    P_.dtargets = nullptr;
    // bf16 MFMA engine buffers (optional: without them only the fp32 kernels can run)
    if (bufs.contains("stage2") && bufs.contains("meta2") && bufs.contains("metaN") && bufs.contains("stepinfo") &&
        bufs.contains("shadow") && bufs.contains("wimg")) {
      P_.stage2 = get("stage2", at::kByte, B * 3072).data_ptr<uint8_t>();
      P_.meta2 = get("meta2", at::kLong, B * 4).data_ptr<int64_t>();
      P_.metaN = get("metaN", at::kLong, B * 4).data_ptr<int64_t>();
      P_.stepinfo = get("stepinfo", at::kLong, 4).data_ptr<int64_t>();
      Tensor sh = bufs["shadow"].cast<Tensor>();
      check_dev(sh, "shadow", at::kShort, 1);
      keep_.push_back(sh);
      P_.shadow = reinterpret_cast<uint16_t*>(sh.data_ptr<int16_t>());
      shadow_n_ = sh.numel();
      P_.wimg = reinterpret_cast<uint16_t*>(get("wimg", at::kShort, lenet_mfma_wimg_elems()).data_ptr<int16_t>());
      TORCH_CHECK(P_.slab1 != nullptr && (int64_t)C1 * 640 >= lenet_mfma_slab_floats(cfg), "slab1 too small");
    }
    if (bufs.contains("trace")) P_.trace = get("trace", at::kFloat, 4096).data_ptr<float>();
    // next-step input prep in the batch-reduction kernel (MLT_LENET_PREP=0: off, for A/B)
    const char* pe = std::getenv("MLT_LENET_PREP");
    if (bufs.contains("prep") && bufs.contains("pmeta") && !(pe && std::string(pe) == "0")) {
      P_.prep = get("prep", at::kByte, B * 8192).data_ptr<uint8_t>();
      P_.pmeta = get("pmeta", at::kLong, B * 4).data_ptr<int64_t>();
    }
    // bf16 per-sample kernel with two blocks per sample where eligible (MLT_LENET_SPLIT=0: off, for A/B)
    const char* se = std::getenv("MLT_LENET_SPLIT");
    split_ = !(se && std::string(se) == "0");
    // ... and the role-D parts per sample of a split launch (MLT_LENET_SPLIT_D: 0 auto, else that ND)
    const char* sd = std::getenv("MLT_LENET_SPLIT_D");
    split_parts_ = 0;
    if (sd && *sd) {
      const int n = std::atoi(sd);
      TORCH_CHECK(lenet_mfma_split_parts_valid(n), "MLT_LENET_SPLIT_D=", sd, ": not a built part count");
      split_parts_ = n;
    }
    A_ = LeNetAug{};
    O_ = LeNetOpt{};
  }

  void set_aug(Tensor data, Tensor perm, Tensor ctrl, Tensor dtargets, int64_t seed, int pad, int flip,
               int batch_stride, std::vector<double> mean, std::vector<double> stdv) {
    A_ = make_aug(data, perm, ctrl, seed, pad, flip, batch_stride, mean, stdv);
    TORCH_CHECK(A_.ctrl != nullptr, "ctrl required");
    check_dev(dtargets, "dtargets", at::kLong, A_.n);
    P_.dtargets = dtargets.data_ptr<int64_t>();
    aug_keep_ = {data, perm, ctrl, dtargets};
    graphs_.clear();
  }

  void clear_aug() {
    A_.data = nullptr;
    P_.dtargets = nullptr;
    graphs_.clear();
  }

  void set_ctrl(Tensor ctrl) {
    check_dev(ctrl, "ctrl", at::kLong, 2, 8);
    A_.ctrl = ctrl.data_ptr<int64_t>();
    ctrl_keep_ = ctrl;
    graphs_.clear();
  }

  void set_opt(Tensor p, Tensor g, c10::optional<Tensor> s1, c10::optional<Tensor> s2, int kind, double lr,
               double momentum, double dampening, double wd, double beta1, double beta2, double eps,
               double lr_decay, double grad_scale, bool nesterov, bool maximize, c10::optional<Tensor> lr_t,
               bool lr_table, std::vector<int64_t> offsets) {
    const int64_t n = p.numel();
    check_dev(p, "p", at::kFloat, n);
    check_dev(g, "g", at::kFloat, n);
    O_ = LeNetOpt{};
    master_ = p;
    pack_ver_ = -1;
    O_.p = p.data_ptr<float>();
    O_.g = g.data_ptr<float>();
    O_.n = n;
    O_.s1 = s1.has_value() ? s1->data_ptr<float>() : nullptr;
    O_.s2 = s2.has_value() ? s2->data_ptr<float>() : nullptr;
    if (s1.has_value()) check_dev(*s1, "s1", at::kFloat, n);
    if (s2.has_value()) check_dev(*s2, "s2", at::kFloat, n);
    O_.h = make_hyper(kind, lr, momentum, dampening, wd, beta1, beta2, eps, lr_decay, grad_scale, nesterov,
                      maximize);
    O_.lr_ptr = nullptr;
    O_.lr_table = lr_table ? 1 : 0;
    if (lr_t.has_value()) {
      check_dev(*lr_t, "lr", at::kFloat, 1, 4);
      O_.lr_ptr = lr_t->data_ptr<float>();
    }
    TORCH_CHECK(!lr_table || O_.lr_ptr, "lr_table requires an lr tensor");
    TORCH_CHECK(offsets.size() == 10, "need the flat offsets of the 10 LeNet tensors");
    const int C1 = cfg_ == LENET_TINY ? 4 : 6, C2 = cfg_ == LENET_TINY ? 8 : 16;
    const int F1 = cfg_ == LENET_TINY ? 64 : 120, F2 = cfg_ == LENET_TINY ? 32 : 84;
    const int64_t sizes[10] = {C1 * 75, C1, C2 * C1 * 25, C2, (int64_t)F1 * C2 * 25, F1, F2 * F1, F2, 10 * F2, 10};
    for (int i = 0; i < 10; ++i) {
      TORCH_CHECK(offsets[i] >= 0 && offsets[i] % 4 == 0 && offsets[i] + sizes[i] <= n,
                  "flat offset ", i, " out of range / misaligned");
      O_.off[i] = offsets[i];
    }
    opt_keep_.clear();
    opt_keep_.push_back(p);
    opt_keep_.push_back(g);
    if (s1.has_value()) opt_keep_.push_back(*s1);
    if (s2.has_value()) opt_keep_.push_back(*s2);
    if (lr_t.has_value()) opt_keep_.push_back(*lr_t);
    graphs_.clear();
  }

  // Data-parallel step (mode & LENET_REDUCE): after the backward kernels, all-reduce the
  // flat gradient (AVG) over the native communicator and apply the flat optimizer with lr /
  // step read from device memory -- all inside the same stream (and graph).
  void set_xgmi(py::object x) {
    if (x.is_none()) {
      xgmi_ = nullptr;
      xgmi_keep_ = py::none();
    } else {
      xgmi_ = &x.cast<PyXgmi&>().raw();
      TORCH_CHECK(xgmi_->ready() && xgmi_->capacity() >= O_.n, "xgmi all-reduce not opened / too small");
      xgmi_keep_ = x;
    }
    graphs_.clear();
  }

  void set_comm(py::object comm) {
    if (comm.is_none()) {
      comm_ = nullptr;
      comm_keep_ = py::none();
    } else {
      comm_ = &comm.cast<PyComm&>().raw();
      comm_keep_ = comm;
    }
    graphs_.clear();
  }

  // 0: fp32 kernels (lenet.hip); 1: bf16 MFMA training step (lenet_mfma.hip; evaluation stays fp32)
  void set_precision(int p) {
    TORCH_CHECK(p == 0 || p == 1, "precision: 0 (fp32) or 1 (bf16)");
    if (p == 1) TORCH_CHECK(P_.shadow && P_.wimg && P_.stage2 && P_.meta2 && P_.metaN && P_.stepinfo,
                            "bf16 engine buffers missing");
    prec_ = p;
    pack_ver_ = -1;
    graphs_.clear();
  }
  int precision() const { return prec_; }
  // bf16 + xGMI: the two-launch data-parallel step (default) or the four-launch one (per-sample
  // kernel, batch reductions, xGMI all-reduce, apply) kept for A/B and bitwise cross-checks
  void set_fused_dp(bool f) {
    fused_dp_ = f;
    graphs_.clear();
  }
  bool fused_dp() const { return fused_dp_; }
  // bf16 training step: two blocks per sample in the per-sample kernel (the launch still falls back
  // to one where the split is not eligible: split_active)
  void set_split(bool s) {
    split_ = s;
    graphs_.clear();
  }
  bool split() const { return split_; }
  // what a bf16 training launch at batch B would do with the current dataset / buffers
  bool split_active(int B) const {
    if (prec_ != 1 || B <= 0 || B > max_b_) return false;
    return lenet_mfma_split_active(split_bits(LENET_FWD | LENET_CE | LENET_BWD), B, P_, A_);
  }
  // role-D parts per sample of a split launch (0: auto; a forced value falls back to the next
  // smaller one where (ND + 1) B blocks do not fit the CUs: split_blocks)
  void set_split_parts(int n) {
    TORCH_CHECK(lenet_mfma_split_parts_valid(n), "set_split_parts: ", n, " is not a built part count");
    split_parts_ = n;
    graphs_.clear();
  }
  int split_parts() const { return split_parts_; }
  // blocks per sample of a bf16 training launch at batch B
  int split_blocks(int B) const {
    if (prec_ != 1 || B <= 0 || B > max_b_) return 1;
    return lenet_mfma_split_blocks(split_bits(LENET_FWD | LENET_CE | LENET_BWD), B, P_, A_);
  }
  // (the switches travel to the bf16 step's launch as internal mode bits; no other kernel sees them)
  int split_bits(int mode) const {
    if (prec_ != 1 || !(mode & LENET_BWD)) return mode;
    return split_ ? mode | (split_parts_ << LENET_SPLITD_SHIFT) : mode | LENET_NOSPLIT;
  }

  void check_mode(int mode, int B) const {
    TORCH_CHECK(B > 0 && B <= max_b_, "batch ", B, " outside [1, ", max_b_, "]");
    if (prec_ == 1 && (mode & LENET_BWD)) {
      TORCH_CHECK((mode & LENET_FWD) && (mode & LENET_CE), "bf16 engine: training steps are FWD|CE|BWD");
      TORCH_CHECK(A_.ctrl != nullptr && O_.g != nullptr, "bf16 engine: set_ctrl / set_opt first");
      TORCH_CHECK(shadow_n_ >= O_.n, "bf16 engine: shadow smaller than the flat parameters");
    }
    TORCH_CHECK(!((mode & LENET_OPT) && (mode & LENET_REDUCE)),
                "LENET_OPT (fused local update) and LENET_REDUCE (all-reduce + update) are exclusive");
    if (mode & LENET_REDUCE) TORCH_CHECK(A_.ctrl != nullptr, "ctrl required for the data-parallel update");
    if (mode & (LENET_OPT | LENET_REDUCE)) TORCH_CHECK(O_.g != nullptr, "set_opt() first");
    if (mode & LENET_OPT) TORCH_CHECK(A_.ctrl != nullptr, "ctrl required for the fused optimizer");
    if ((mode & LENET_OPT) && O_.lr_table) TORCH_CHECK(A_.ctrl != nullptr, "lr table needs ctrl");
  }

  void run(int mode, int B) {
    check_mode(mode, B);
    const bool mf = prec_ == 1 && (mode & LENET_BWD);
    if (mf) launch_lenet_mfma_pack(cfg_, P_, O_, cur_stream());  // shadow / fragment image from the masters
    launch_step(cfg_, split_bits(mode), B, P_, A_, O_, comm_, xgmi_, cur_stream(), mf, fused_dp_);
  }

  // transport bring-up: the batch reductions of the current activation / slab buffers into the
  // flat gradient (exchange = the fused xGMI exchange too), no update, step counters untouched
  void reduce_only(int B, bool exchange) {
    TORCH_CHECK(prec_ == 1 && P_.stepinfo && O_.g, "reduce_only: bf16 engine with set_opt");
    TORCH_CHECK(B > 0 && B <= max_b_, "reduce_only: batch");
    if (exchange) {
      TORCH_CHECK(xgmi_ != nullptr, "reduce_only: no xGMI transport");
      const XgmiFused X = xgmi_->fused_view();
      launch_lenet_mfma_reduce(cfg_, B, P_, O_, &X, cur_stream());
    } else {
      launch_lenet_mfma_reduce(cfg_, B, P_, O_, nullptr, cur_stream());
    }
  }

  static void launch_step(int cfg, int mode, int B, const LeNetPtrs& P, const LeNetAug& A, const LeNetOpt& O,
                          Communicator* comm, XgmiAllReduce* xgmi, hipStream_t s, bool mfma = false,
                          bool fused_dp = false) {
    if (mfma && (mode & LENET_REDUCE) && xgmi && fused_dp) {
      // bf16 data-parallel step in two launches: the per-sample kernel, then batch reductions +
      // xGMI exchange + rank-ordered sum + update (lenet_mwx; world size 1 = loopback)
      launch_lenet_mfma_dp(cfg, mode & ~LENET_REDUCE, B, P, A, O, xgmi->fused_view(), s);
      return;
    }
    if (mfma) {
      launch_lenet_mfma(cfg, mode & ~LENET_REDUCE, B, P, A, O, s);
    } else {
      launch_lenet(cfg, mode & ~LENET_REDUCE, B, P, A, O, s);
    }
    if (mode & LENET_REDUCE) {
      if (xgmi && xgmi->world() > 1) {
        // xGMI all-reduce of the latency-bound bucket, then the flat update VETOED by the
        // transport's sticky error word: a step with any timed-out slice is applied on no slice
        // of this rank (all-or-nothing; the host raises TransportError after the replay)
        xgmi->launch(O.g, O.n, 1.f / xgmi->world(), s, nullptr);
        if (mfma) {  // bf16: update + shadow + fragment images in one launch, vetoed like the flat update
          launch_lenet_mfma_apply(cfg, P, O, xgmi->error_dev(), s);
          return;
        }
        launch_flat_optim(O.p, O.g, O.s1, O.s2, O.n, O.h, O.lr_ptr, O.lr_table ? A.ctrl + 1 : nullptr, A.ctrl, 1.0,
                          nullptr, nullptr, s, xgmi->error_dev());
        return;
      }
      if (comm)  // (size 1 too: the W=1 RCCL rehearsal captures a real ncclAllReduce)
        comm->all_reduce(O.g, O.g, (size_t)O.n, CommDtype::F32, CommOp::AVG, s);
      if (mfma) {  // the bf16 step reads its weights from the shadow / fragment images: one apply launch
        launch_lenet_mfma_apply(cfg, P, O, nullptr, s);
        return;
      }
      // ctrl[0] = steps taken (already advanced by the backward kernel) -> Adam t; ctrl[1] -> lr table index
      launch_flat_optim(O.p, O.g, O.s1, O.s2, O.n, O.h, O.lr_ptr, O.lr_table ? A.ctrl + 1 : nullptr, A.ctrl, 1.0,
                        nullptr, nullptr, s);
    }
  }

  // Capture `nsteps` consecutive steps (the device step counter advances inside)
  void capture(int mode, int B, int nsteps) {
    check_mode(mode, B);
    TORCH_CHECK(nsteps >= 1 && nsteps <= 4096, "nsteps");
    TORCH_CHECK((mode & LENET_BWD) == 0 || A_.ctrl != nullptr || nsteps == 1,
                "multi-step capture needs the device step counter");
    auto g = std::make_unique<HipGraph>();
    const LeNetPtrs P = P_;
    const LeNetAug A = A_;
    const LeNetOpt O = O_;
    const int cfg = cfg_;
    Communicator* comm = comm_;
    XgmiAllReduce* xgmi = xgmi_;
    const bool mf = prec_ == 1 && (mode & LENET_BWD);
    const bool fused = fused_dp_;
    const int lmode = split_bits(mode);
    g->capture([&](hipStream_t s) {
      // (no pack here: replay() re-packs when the host changed the masters since the last pack)
      for (int i = 0; i < nsteps; ++i) launch_step(cfg, lmode, B, P, A, O, comm, xgmi, s, mf, fused);
    });
    graphs_[key(mode, B, nsteps)] = std::move(g);
  }

  bool has_graph(int mode, int B, int nsteps) const { return graphs_.count(key(mode, B, nsteps)) != 0; }

  // bf16 engine: the step kernels read the bf16 shadow / fragment images, which they keep in step
  // with the fp32 masters themselves. A host-side change of the masters (any torch in-place op:
  // the flat buffer's version counter moves; invalidate_shadow() for native writers) is folded in
  // by one pack launch ahead of the next replay.
  void sync_shadow() {
    if (prec_ != 1 || !master_.defined()) return;
    const int64_t v = master_._version();
    if (v == pack_ver_) return;
    launch_lenet_mfma_pack(cfg_, P_, O_, cur_stream());
    pack_ver_ = v;
  }
  void invalidate_shadow() { pack_ver_ = -1; }

  void replay(int mode, int B, int nsteps) {
    auto it = graphs_.find(key(mode, B, nsteps));
    TORCH_CHECK(it != graphs_.end(), "no captured graph for this (mode, B, nsteps)");
    if (mode & LENET_BWD) sync_shadow();
    it->second->launch(cur_stream());
  }

  size_t graph_nodes(int mode, int B, int nsteps) const {
    auto it = graphs_.find(key(mode, B, nsteps));
    return it == graphs_.end() ? 0 : it->second->num_nodes();
  }

  void reset_graphs() { graphs_.clear(); }

 private:
  static int64_t key(int mode, int B, int nsteps) {
    return ((int64_t)mode << 48) | ((int64_t)B << 16) | (int64_t)nsteps;
  }
  int cfg_;
  int max_b_;
  LeNetPtrs P_{};
  LeNetAug A_{};
  LeNetOpt O_{};
  std::vector<Tensor> keep_, aug_keep_, opt_keep_;
  Tensor ctrl_keep_;
  Communicator* comm_ = nullptr;
  py::object comm_keep_ = py::none();
  XgmiAllReduce* xgmi_ = nullptr;
  py::object xgmi_keep_ = py::none();
  std::map<int64_t, std::unique_ptr<HipGraph>> graphs_;
  int prec_ = 0;
  bool fused_dp_ = true;
  bool split_ = true;
  int split_parts_ = 0;
  int64_t shadow_n_ = 0;
  Tensor master_;          // the fp32 masters (version counter: host-side changes)
  int64_t pack_ver_ = -1;  // master_._version() at the last pack
};

}  // namespace mlt

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  using namespace mlt;
  m.doc() = "ml_trainer_amd native gfx950 kernels and runtime";
  m.attr("ARCH") = "gfx950";
  m.def("flat_optim", &flat_optim, py::arg("p"), py::arg("g"), py::arg("s1"), py::arg("s2"), py::arg("kind"),
        py::arg("lr"), py::arg("momentum"), py::arg("dampening"), py::arg("weight_decay"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("lr_decay"), py::arg("grad_scale"), py::arg("nesterov"),
        py::arg("maximize"), py::arg("lr_t") = py::none(), py::arg("lr_index") = py::none(),
        py::arg("step_t") = py::none(), py::arg("t_host") = 1.0, py::arg("shadow") = py::none(),
        py::arg("coef") = py::none());
  m.def("optim_chunk_elems", &optim_chunk_elems);
  m.def("flat_optim_seg", &flat_optim_seg, py::arg("p"), py::arg("g"), py::arg("s1"), py::arg("s2"),
        py::arg("chunks"), py::arg("wd"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("grad_scale"), py::arg("maximize"), py::arg("lr_t") = py::none(), py::arg("lr_index") = py::none(),
        py::arg("step_t") = py::none(), py::arg("t_host") = 1.0, py::arg("shadow") = py::none(),
        py::arg("coef") = py::none(), py::arg("skip") = py::none(), py::arg("max_blocks") = 0);
  m.def("lamb_step", &lamb_step, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("chunks"),
        py::arg("tseg"), py::arg("wd"), py::arg("adapt"), py::arg("part"), py::arg("norms"), py::arg("trust"),
        py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("grad_scale"),
        py::arg("maximize"), py::arg("lr_t") = py::none(), py::arg("lr_index") = py::none(),
        py::arg("step_t") = py::none(), py::arg("t_host") = 1.0, py::arg("shadow") = py::none(),
        py::arg("coef") = py::none(), py::arg("skip") = py::none(), py::arg("max_blocks") = 0,
        py::arg("stages") = 7);
  m.def("sq_norm", &sq_norm);
  m.def("clip_coef", &clip_coef);
  m.def("cast_bf16", &cast_bf16);
  m.def("transpose_bf16", &transpose_bf16);
  m.def("cifar_augment", &cifar_augment);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("head_cls_fwd", &head_cls_fwd, py::arg("pooled"), py::arg("wc"), py::arg("bc"), py::arg("logits"));
  m.def("head_cls_bwd", &head_cls_bwd, py::arg("dlogits"), py::arg("pooled"), py::arg("wc"), py::arg("dpre"),
        py::arg("dwc"), py::arg("dbc"), py::arg("accumulate") = false);
  m.def("accuracy", &accuracy);
  m.def("pointwise_loss_fwd", &pointwise_loss_fwd);
  m.def("nll_fwd", &nll_fwd);
  m.def("loss_scale_grad", &loss_scale_grad);
  m.def("nll_bwd", &nll_bwd);
  m.def("mcrmse", &mcrmse);
  m.def("loss_partials_needed", &loss_partials_needed);
  m.def("gemm", &gemm, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("a_mn"), py::arg("b_mn"),
        py::arg("bias") = py::none(), py::arg("aux") = py::none(), py::arg("res") = py::none(),
        py::arg("alpha") = 1.0, py::arg("mode") = 0, py::arg("accumulate") = false, py::arg("cfg") = -1,
        py::arg("splits") = 0, py::arg("colsum_out") = py::none(), py::arg("colsum_accumulate") = false);
  m.def("gemm_skinny", &gemm_skinny, py::arg("X"), py::arg("W"), py::arg("Y"), py::arg("bias") = py::none(),
        py::arg("aux") = py::none(), py::arg("res") = py::none(), py::arg("mode") = 0);
  m.def("gemm_skinny_max_rows", []() { return kSkinnyMaxRows; });
  m.def("gemm_f8", &gemm_f8, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("fmt_a"), py::arg("fmt_b"),
        py::arg("inv_scale_a"), py::arg("inv_scale_b"), py::arg("bias") = py::none(), py::arg("aux") = py::none(),
        py::arg("res") = py::none(), py::arg("alpha") = 1.0, py::arg("mode") = 0, py::arg("accumulate") = false,
        py::arg("cfg") = -1, py::arg("splits") = 0);
  m.def("gemm_f8_q", &gemm_f8_q, py::arg("A"), py::arg("B"), py::arg("Y"), py::arg("Yt"), py::arg("fmt_a"),
        py::arg("fmt_b"), py::arg("inv_scale_a"), py::arg("inv_scale_b"), py::arg("out_fmt"), py::arg("out_scale"),
        py::arg("out_amax"), py::arg("bias") = py::none(), py::arg("aux") = py::none(), py::arg("mode") = 0,
        py::arg("colsum_out") = py::none(), py::arg("colsum_accumulate") = false);
  m.def("gemm_f8_plan", [](int64_t M, int64_t N, int64_t K, int cfg, int splits) {
    check_gemm_cfg(cfg);
    const GemmPlan p = plan_gemm_f8((int)M, (int)N, (int)K, cfg, splits);
    return py::make_tuple(p.cfg, p.splits, p.ksteps, p.ws_floats, p.ext);
  }, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("cfg") = -1, py::arg("splits") = 0);
  m.def("set_gemm_split_mode", &set_gemm_split_mode, py::arg("mode"));
  m.def("set_gemm_w4q8", &set_gemm_w4q8, py::arg("on"));
  m.def("lenet_mfma_wimg_elems", &lenet_mfma_wimg_elems);
  m.def("lenet_mfma_trace_build", &lenet_mfma_trace_build);
  // host-side completion waits of a device: spin (lowest latency; the launch-bound LeNet step
  // syncs per epoch / per timed region) instead of ROCm's default yield. Call before the device's
  // context is active; returns the hipError_t (hipErrorSetOnActiveProcess: too late, unchanged).
  m.def("set_device_sync_spin", [](int device) {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipSetDeviceFlags(hipDeviceScheduleSpin);
    return (int)e;
  });
  m.def("lenet_mfma_slab_floats", &lenet_mfma_slab_floats, py::arg("cfg"));
  m.def("lenet_mfma_kw_blocks", &lenet_mfma_kw_blocks, py::arg("cfg"));
  m.def("lenet_mfma_xch_granules", &lenet_mfma_xch_granules, py::arg("cfg"));
  m.def("fp8_cast", &fp8_cast, py::arg("x"), py::arg("y"), py::arg("scale"), py::arg("amax") = py::none(),
        py::arg("fmt") = 0);
  m.def("fp8_amax", &fp8_amax);
  m.def("fp8_cast_transpose", &fp8_cast_transpose, py::arg("w"), py::arg("y"), py::arg("yt"), py::arg("scale"),
        py::arg("amax") = py::none(), py::arg("fmt") = 0, py::arg("colsum_out") = py::none(),
        py::arg("colsum_accumulate") = false);
  m.attr("FP8_AMAX_SLOTS") = kAmaxSlots * kAmaxStride;  // floats of amax state per tensor
  m.def("fp8_update_scale", &fp8_update_scale, py::arg("hist"), py::arg("amax"), py::arg("scale"),
        py::arg("inv_scale"), py::arg("fmax"), py::arg("step"), py::arg("margin") = 0);
  m.def("gemm_plan", &gemm_plan, py::arg("a_mn"), py::arg("b_mn"), py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("cfg") = -1, py::arg("splits") = 0, py::arg("accumulate") = false);
  m.def("colsum", &colsum, py::arg("X"), py::arg("out"), py::arg("accumulate") = false);
  m.def("vocab_ce", &vocab_ce, py::arg("Z"), py::arg("V"), py::arg("labels"), py::arg("row_loss"), py::arg("row_lse"),
        py::arg("row_hit"), py::arg("write_grad"), py::arg("ignore_index") = -100);
  m.def("vocab_ce_resident_cols", &vocab_ce_resident_cols);
  m.def("mlm_select", &mlm_select, py::arg("labels"), py::arg("P"), py::arg("slot_row"), py::arg("slot_label"),
        py::arg("seq_overflow"), py::arg("overflow"), py::arg("lens") = py::none(),
        py::arg("cu_seqlens") = py::none(), py::arg("ignore_index") = -100);
  m.def("gather_rows", &gather_rows, py::arg("X"), py::arg("slot_row"), py::arg("out"));
  m.def("scatter_rows", &scatter_rows, py::arg("G"), py::arg("slot_row"), py::arg("dX"));
  m.def("ln_fwd", &ln_fwd);
  m.def("ln_bwd", &ln_bwd, py::arg("DY"), py::arg("X"), py::arg("gamma"), py::arg("mean"), py::arg("rstd"),
        py::arg("DX"), py::arg("part"), py::arg("dgamma"), py::arg("dbeta"), py::arg("accumulate") = false,
        py::arg("dres") = py::none(), py::arg("dxsum") = py::none(), py::arg("dxsum_acc") = false,
        py::arg("dxm") = py::none(), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("site") = 0,
        py::arg("rank") = 0);
  m.def("dropout", &dropout, py::arg("x"), py::arg("out"), py::arg("p"), py::arg("seed"), py::arg("site"),
        py::arg("rank"));
  m.def("dropout_add_ln_fwd", &dropout_add_ln_fwd, py::arg("Y0"), py::arg("RES"), py::arg("gamma"), py::arg("beta"),
        py::arg("Z"), py::arg("Y"), py::arg("mean"), py::arg("rstd"), py::arg("eps"), py::arg("p"), py::arg("seed"),
        py::arg("site"), py::arg("rank"));
  m.def("ln_partial_blocks", &ln_partial_blocks);
  m.def("ln_bwd_dropout_res", &ln_bwd_dropout_res, py::arg("DY"), py::arg("X"), py::arg("gamma"), py::arg("mean"),
        py::arg("rstd"), py::arg("DX"), py::arg("part"), py::arg("dgamma"), py::arg("dbeta"), py::arg("accumulate"),
        py::arg("dres"), py::arg("dxsum"), py::arg("dxsum_acc"), py::arg("dxm"), py::arg("p"), py::arg("seed"),
        py::arg("site"), py::arg("rank"));
  m.def("rms_fwd", &rms_fwd, py::arg("X"), py::arg("gamma"), py::arg("Y"), py::arg("rstd"), py::arg("eps"));
  m.def("dropout_add_rms_fwd", &dropout_add_rms_fwd, py::arg("Y0"), py::arg("RES"), py::arg("gamma"), py::arg("Z"),
        py::arg("Y"), py::arg("rstd"), py::arg("eps"), py::arg("p"), py::arg("seed"), py::arg("site"),
        py::arg("rank"));
  m.def("rms_bwd", &rms_bwd, py::arg("DY"), py::arg("X"), py::arg("gamma"), py::arg("rstd"), py::arg("DX"),
        py::arg("part"), py::arg("dgamma"), py::arg("accumulate") = false, py::arg("dres") = py::none(),
        py::arg("dxsum") = py::none(), py::arg("dxsum_acc") = false, py::arg("dxm") = py::none(), py::arg("p") = 0.0,
        py::arg("seed") = 0, py::arg("site") = 0, py::arg("rank") = 0);
  m.def("embed_fwd", &embed_fwd, py::arg("ids"), py::arg("tt"), py::arg("Ww"), py::arg("Wp"), py::arg("Wt"),
        py::arg("out"), py::arg("S"), py::arg("pos") = py::none());
  m.def("embed_bwd", &embed_bwd, py::arg("sid"), py::arg("perm"), py::arg("tt"), py::arg("DX"), py::arg("gw"),
        py::arg("gp"), py::arg("gt"), py::arg("part"), py::arg("S"), py::arg("cu_seqlens") = py::none());
  m.def("attn_fwd", &attn_fwd, py::arg("qkv"), py::arg("out"), py::arg("lse"), py::arg("lens"), py::arg("B"),
        py::arg("S"), py::arg("H"), py::arg("scale"), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("site") = 0,
        py::arg("rank") = 0, py::arg("cu_seqlens") = py::none(), py::arg("causal") = false);
  m.def("sample_step", &sample_step, py::arg("logits"), py::arg("V"), py::arg("params"), py::arg("draws"),
        py::arg("seq_ids"), py::arg("finished"), py::arg("lengths"), py::arg("tokens"), py::arg("next_ids"),
        py::arg("n_kept"));
  m.def("sample_weights", &sample_weights, py::arg("logits"), py::arg("V"), py::arg("inv_t_log2e"));
  m.def("attn_decode", &attn_decode, py::arg("qkv_new"), py::arg("kv"), py::arg("pos"), py::arg("out"), py::arg("H"),
        py::arg("scale"), py::arg("rope") = py::none());
  m.def("rope_qk", &rope_qk, py::arg("qkv"), py::arg("table"), py::arg("H"), py::arg("S"), py::arg("pos") = py::none(),
        py::arg("sign") = 1);
  m.def("attn_bwd", &attn_bwd, py::arg("qkv"), py::arg("out"), py::arg("dout"), py::arg("lse"), py::arg("delta"),
        py::arg("lens"), py::arg("dqkv"), py::arg("B"), py::arg("S"), py::arg("H"), py::arg("scale"),
        py::arg("colsum_out") = py::none(), py::arg("colsum_accumulate") = false, py::arg("q8_y") = py::none(),
        py::arg("q8_yt") = py::none(), py::arg("q8_scale") = py::none(), py::arg("q8_amax") = py::none(),
        py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("site") = 0, py::arg("rank") = 0,
        py::arg("cu_seqlens") = py::none(), py::arg("causal") = false);
  py::class_<PyComm>(m, "Communicator")
      .def(py::init<py::bytes, int, int, int>(), py::arg("unique_id"), py::arg("nranks"), py::arg("rank"),
           py::arg("device"))
      .def_static("unique_id", &PyComm::unique_id)
      .def_property_readonly("rank", &PyComm::rank)
      .def_property_readonly("size", &PyComm::size)
      .def("all_reduce", &PyComm::all_reduce, py::arg("tensor"), py::arg("op") = "sum")
      .def("reduce_scatter", &PyComm::reduce_scatter, py::arg("input"), py::arg("output"), py::arg("op") = "sum")
      .def("all_gather", &PyComm::all_gather, py::arg("input"), py::arg("output"))
      .def("broadcast", &PyComm::broadcast, py::arg("tensor"), py::arg("root") = 0)
      .def("all_to_all", &PyComm::all_to_all, py::arg("input"), py::arg("output"))
      .def("async_error", &PyComm::async_error)
      .def("abort", &PyComm::abort);
  py::class_<PyXgmi>(m, "XgmiAllReduce", py::dynamic_attr())
      .def(py::init<int64_t, int, int, int, int>(), py::arg("capacity"), py::arg("world"), py::arg("rank"),
           py::arg("device"), py::arg("blocks") = 64)
      .def("handle", &PyXgmi::handle)
      .def("open", &PyXgmi::open)
      .def("all_reduce", &PyXgmi::all_reduce, py::arg("tensor"), py::arg("average") = true)
      .def("error", &PyXgmi::error)
      .def_property_readonly("world", [](PyXgmi& x) { return x.raw().world(); })
      .def_property("timeout_ms", &PyXgmi::timeout_ms, &PyXgmi::set_timeout_ms)
      .def_property("algo", &PyXgmi::algo, &PyXgmi::set_algo)
      .def_property("fault", &PyXgmi::fault, &PyXgmi::set_fault)
      .def_property("fused_two", &PyXgmi::fused_two, &PyXgmi::set_fused_two);
  py::class_<PyPrefetcher>(m, "PinnedPrefetcher")
      .def(py::init<int64_t, int, int>(), py::arg("slot_bytes"), py::arg("depth"), py::arg("device"))
      .def("slot", &PyPrefetcher::slot)
      .def("copy_to_device", &PyPrefetcher::copy_to_device)
      .def("acquire", &PyPrefetcher::acquire)
      .def("release", &PyPrefetcher::release)
      .def("ready", &PyPrefetcher::ready)
      .def("wait", &PyPrefetcher::wait)
      .def_property_readonly("depth", &PyPrefetcher::depth)
      .def_property_readonly("slot_bytes", &PyPrefetcher::slot_bytes);
  py::class_<LeNetEngine>(m, "LeNetEngine")
      .def(py::init<int, int, py::dict>())
      .def("set_aug", &LeNetEngine::set_aug)
      .def("set_comm", &LeNetEngine::set_comm)
      .def("set_xgmi", &LeNetEngine::set_xgmi)
      .def_property("fused_dp", &LeNetEngine::fused_dp, &LeNetEngine::set_fused_dp)
      .def("set_split", &LeNetEngine::set_split)
      .def("split", &LeNetEngine::split)
      .def("split_active", &LeNetEngine::split_active, py::arg("B"))
      .def("set_split_parts", &LeNetEngine::set_split_parts, py::arg("n"))
      .def("split_parts", &LeNetEngine::split_parts)
      .def("split_blocks", &LeNetEngine::split_blocks, py::arg("B"))
      .def("clear_aug", &LeNetEngine::clear_aug)
      .def("set_ctrl", &LeNetEngine::set_ctrl)
      .def("set_opt", &LeNetEngine::set_opt)
      .def("set_precision", &LeNetEngine::set_precision)
      .def("precision", &LeNetEngine::precision)
      .def("run", &LeNetEngine::run)
      .def("capture", &LeNetEngine::capture)
      .def("has_graph", &LeNetEngine::has_graph)
      .def("replay", &LeNetEngine::replay)
      .def("invalidate_shadow", &LeNetEngine::invalidate_shadow)
      .def("reduce_only", &LeNetEngine::reduce_only, py::arg("B"), py::arg("exchange"))
      .def("graph_nodes", &LeNetEngine::graph_nodes)
      .def("reset_graphs", &LeNetEngine::reset_graphs);
  m.attr("LENET_FWD") = (int)LENET_FWD;
  m.attr("LENET_CE") = (int)LENET_CE;
  m.attr("LENET_BWD") = (int)LENET_BWD;
  m.attr("LENET_OPT") = (int)LENET_OPT;
  m.attr("LENET_TRACE") = (int)LENET_TRACE;
  m.attr("LENET_REDUCE") = (int)LENET_REDUCE;
}
