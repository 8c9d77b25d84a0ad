// Optimizer math shared by the W&D kernels (csrc/wd_tail.h reductions + optimizers, csrc/wd_chain.hip's
// in-kernel tail): TF ApplyAdagrad / ApplyFtrl / Adam / SGD on one fp32 parameter (no epsilon in Adagrad, as TF),
// and the slab-column-order state (param / s0 / s1 indexed by gradient column; wsc[col]: -1 padding, -2 wide weight,
// >= 0 DNN weight with its bf16 weight-image offset). Included inside each translation unit's anonymous namespace.
#pragma once

struct OptHyper {
  int kind;        // 0 sgd, 1 adagrad, 2 ftrl, 3 adam
  float lr, beta1, beta2, eps, l1, l2, lr_power;
};
// the launchers' hyper_dnn / hyper_wide arguments: 8 host floats in the order of the fields
inline OptHyper opt_hyper(const float* h) { return OptHyper{(int)h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]}; }

__device__ __forceinline__ float opt_update(const OptHyper& hp, float w, float g, float& a0, float& a1,
                                            long long step) {
  if (hp.kind == 0) return w - hp.lr * g;
  if (hp.kind == 1) {
    a0 += g * g;
    return w - hp.lr * g * rsqrtf(a0);
  }
  if (hp.kind == 2) {  // TF ApplyFtrl
    const float a = a0, an = a + g * g;
    float sq_new, sq_old;
    if (hp.lr_power == -0.5f) {
      sq_new = sqrtf(an);
      sq_old = sqrtf(a);
    } else {
      sq_new = powf(an, -hp.lr_power);
      sq_old = powf(a, -hp.lr_power);
    }
    a1 += g - (sq_new - sq_old) / hp.lr * w;
    const float quad = sq_new / hp.lr + 2.f * hp.l2;
    a0 = an;
    return fabsf(a1) > hp.l1 ? (copysignf(hp.l1, a1) - a1) / quad : 0.f;
  }
  {
    // Adam: every operation rounded on its own. With FMA contraction the compiler fuses these sums of products
    // differently from kernel to kernel ((1 - beta) * g became fma(-beta, g, g) in wd_res_opt_sc and a packed multiply
    // in wd_opt1_sc), and the variants of one step then disagree in the last bits of the moments
    // (tests/test_wd_optimizer.py asserts that they are bit-identical).
#pragma clang fp contract(off)
    a0 = hp.beta1 * a0 + (1.f - hp.beta1) * g;
    a1 = hp.beta2 * a1 + (1.f - hp.beta2) * g * g;
    const float bc1 = 1.f - powf(hp.beta1, (float)step);
    const float bc2 = 1.f - powf(hp.beta2, (float)step);
    return w - hp.lr * (a0 / bc1) / (sqrtf(a1 / bc2) + hp.eps);
  }
}

// per-workgroup optimizer step slots (see csrc/wd_tail.h)
constexpr int STEP_SLOTS = 512;

struct ScState {
  int w;           // wsc entry
  float p, a0, a1;
};
// The four loads are unconditional, at the column clamped into [0, stride): straight-line code with no branch per
// load, so they are issued back to back with whatever the caller loads next to them. A thread past the last column
// gets w = -1 (padding) and stores nothing.
__device__ __forceinline__ ScState sc_load(int gi, int stride, const int* __restrict__ wsc, const float* __restrict__ param,
                                           const float* __restrict__ s0, const float* __restrict__ s1) {
  const int gc = min(gi, stride - 1);
  ScState st{wsc[gc], param[gc], s0[gc], s1[gc]};
  if (gi >= stride) st.w = -1;
  return st;
}
// The one point where a column's loads are consumed, placed by the kernel after everything it needs has been issued:
// the state, the step slot, and wt_out and both hyper-parameter structs (kernel arguments past the preloaded dwords) must be in
// registers here, so the compiler can neither sink the state loads into the branch of sc_update that uses them nor
// start the hyper-parameter load only there -- one wait for one round trip, then the update runs from registers.
// NG: the gradient words the kernel loaded beside the state (1 slab entry, 8 partials), landed at the same point.
template <int NG>
__device__ __forceinline__ void sc_landed(ScState& st, float (&g)[NG], long long& step, const uint16_t* wt_out, OptHyper& hd,
                                          OptHyper& hw) {
  static_assert(NG == 1 || NG == 8, "gradient words per column");
  asm volatile(""
               : "+v"(st.w), "+v"(st.p), "+v"(st.a0), "+v"(st.a1), "+s"(step), "+s"(hd.kind), "+s"(hd.lr),
                 "+s"(hd.beta1), "+s"(hd.beta2), "+s"(hd.eps), "+s"(hd.l1), "+s"(hd.l2), "+s"(hd.lr_power),
                 "+s"(hw.kind), "+s"(hw.lr), "+s"(hw.beta1), "+s"(hw.beta2), "+s"(hw.eps), "+s"(hw.l1), "+s"(hw.l2),
                 "+s"(hw.lr_power), "+v"(g[0])
               : "s"(wt_out));  // (an input only: the pointer keeps its global address space)
  if constexpr (NG == 8)
    asm volatile("" : "+v"(g[1]), "+v"(g[2]), "+v"(g[3]), "+v"(g[4]), "+v"(g[5]), "+v"(g[6]), "+v"(g[7]));
}
// wsc == -1 (padding) decides the update and its stores only; sc_load's loads never depend on it
__device__ __forceinline__ void sc_update(int gi, ScState st, float g, const OptHyper& hd, const OptHyper& hw,
                                          long long step, float* __restrict__ param, float* __restrict__ s0,
                                          float* __restrict__ s1, uint16_t* __restrict__ wt_out) {
  if (st.w == -1) return;
  const float w = opt_update(st.w >= 0 ? hd : hw, st.p, g, st.a0, st.a1, step);
  s0[gi] = st.a0;
  s1[gi] = st.a1;
  param[gi] = w;
  if (st.w >= 0) wt_out[st.w] = __builtin_bit_cast(uint16_t, (bf16)w);
}

