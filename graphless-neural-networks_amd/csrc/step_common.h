// Host-side pieces that the one-call training steps share (sage_step.hip, sage_mean_step.hip, mlp_step.hip).  `who` is the calling entry's
// name: every error text starts with it.
#pragma once
#include "glnn_common.h"

namespace glnn {

// A whole optimisation step: fwd_bwd(pf), then the fused Adam launch on the same stream.  The descriptor is checked before anything is
// launched.  may_fold: the backward can leave its last partial sums to Adam -- it then gets a PendingFolds to register them in (NULL under
// GLNN_STUDENT_ADAM_FOLDS=0 or with more than 32 tensors: it folds them itself).
template <class FwdBwd>
inline int step_then_adam(const glnn_adam_desc* adam, const char* who, bool may_fold, void* stream, FwdBwd&& fwd_bwd) {
  GLNN_REQUIRE(adam && adam->params && adam->grads && adam->exp_avg && adam->exp_avg_sq && adam->sizes && adam->grads_host,
               "%s: the Adam descriptor is incomplete", who);
  PendingFolds pf = {};
  const bool folds = may_fold && opts().adam_folds && adam->num_tensors <= 32;
  GLNN_TRY(fwd_bwd(folds ? &pf : nullptr));
  return adam_step(adam->params, adam->grads, adam->exp_avg, adam->exp_avg_sq, adam->sizes, adam->num_tensors, adam->max_size, adam->lr,
                   adam->beta1, adam->beta2, adam->eps, adam->weight_decay, adam->step, adam->grads_host, folds ? &pf : nullptr, stream);
}

// the LayerNorm side descriptor of a sampled-block SAGE step (`d` has L layers, so L - 1 hidden tails)
inline int check_sage_ln_desc(const glnn_sage_step_desc* d, const glnn_sage_ln_desc* ln, const char* who) {
  GLNN_REQUIRE(!d->batchnorm && ln->eps > 0.f, "%s: LayerNorm tails need batchnorm == 0 and eps > 0", who);
  for (int l = 0; l < d->num_layers - 1; ++l) {
    const glnn_sage_ln_layer& q = ln->layer[l];
    GLNN_REQUIRE(q.gamma && q.beta && q.ggamma && q.gbeta && q.mean && q.rstd, "%s: LayerNorm of hidden layer %d: null pointer", who, l);
  }
  return GLNN_OK;
}

// The tail of hidden layer l behind its projection z_l.  LayerNorm (ln != NULL): the row statistics of z, and h = tail(z) too when it is
// materialised.  Otherwise the BatchNorm statistics (cs.done: their first pass is the producing GEMM's epilogue) and, with an h buffer,
// h = tail(z); with h == NULL the next layer's gather evaluates the tail itself (source_tail_dev.h).
inline int sage_hidden_tail_fwd(const glnn_sage_step_desc* d, const glnn_sage_ln_desc* ln, int l, const ColStats& cs, void* stream) {
  const glnn_sage_layer& y = d->layer[l];
  const int d_out = d->dims[l + 1];
  const float p = d->dropout_p;
  if (ln) {
    const glnn_sage_ln_layer& q = ln->layer[l];
    return glnn_layernorm_fwd_f32(y.z, y.ldz, y.n_dst, d_out, q.gamma, q.beta, ln->eps, 1, p, y.drop_seed, y.h, y.ldh, q.mean, q.rstd, stream);
  }
  if (d->batchnorm)
    GLNN_TRY(bn_stats(y.z, y.ldz, y.n_dst, d_out, y.gamma, y.beta, d->bn_eps, d->bn_momentum, y.running_mean, y.running_var, y.nbt, y.mean,
                      y.rstd, y.a_scale, y.a_shift, d->ws_bn, d->ws_bn_floats, stream, nullptr, nullptr, nullptr, 0, nullptr,
                      cs.done ? &cs : nullptr));
  if (y.h)
    GLNN_TRY(glnn_act_fwd_f32(y.z, y.ldz, y.n_dst, d_out, d->batchnorm ? y.a_scale : nullptr, d->batchnorm ? y.a_shift : nullptr, p,
                              y.drop_seed, y.h, y.ldh, stream));
  return GLNN_OK;
}

}  // namespace glnn
