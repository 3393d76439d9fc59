// The per-element optimizer arithmetic shared by the touched-row updates / dense sweeps (optim.hip)
// and the deferred replay (replay.hip).  Both include it after `#pragma clang fp contract(off)`
// and are compiled with -fno-slp-vectorize (csrc/Makefile), so a function here gives the same
// operations, hence the same bits, in both.
#pragma once

#include "kernels.h"

namespace ttamm {

namespace {

// torch single-tensor Adam/AdamW (adam.py:419-547):
//   p *= 1 - lr*wd ; m.lerp_(g, 1-b1) ; v = v*b2 + (1-b2)*g*g ;
//   p += -step * m / (sqrt(v)/sqrt(bc2) + eps)
// G0: the gradient is the literal 0 (an untouched dense-table row): lerp(m, 0, w) =
// m + w*(0 - m) == fma(w, -m, m) and v*b2 + (1-b2)*0*0 == v*b2 (v >= +0), bit for bit.
// FAST (g = 0 rows only, ttamm.h TTAMM_G0_FAST): sqrt and 1/denom from v_sqrt_f32 / v_rcp_f32
// (<= 1 ulp each) and a multiply by RN(1 / sqrt(bc2)) — a third of the IEEE sequences' VALU work.
template <bool DECOUPLED, bool G0 = false, bool FAST = false>
__device__ __forceinline__ void adam_elem_t(float& p, float& m, float& v, float g, const AdamConsts& c) {
    if (DECOUPLED) {
        p = p * c.decay;
    } else if (c.wd != 0.f) {
        g = g + p * c.wd;
    }
    if (G0 && DECOUPLED) {
        m = fmaf(c.w1, -m, m);
        v = v * c.b2;
    } else {
        m = fmaf(c.w1, g - m, m);  // ATen lerp (|w| < 0.5): self + w * (end - self), vectorised as fmadd
        v = v * c.b2;
        v = v + c.w2 * g * g;
    }
    if constexpr (FAST) {
        static_assert(G0, "fast arithmetic is for the g = 0 updates only");
        // the step folded into the reciprocal: r = neg_step / denom = rcp(sqrt(v) * fast_ibc +
        // fast_eps), p = fma(m, r, p): one multiply fewer per element than m * rcp(denom) scaled
        // by neg_step, and the denominator's fma pairs into v_pk_fma_f32 (replay_kernel).  The
        // replay is VALU-issue-bound.  m and v stay bit-exact (torch's operations); p moves by the
        // same update term within a few ulp.
        const float d = fmaf(__builtin_amdgcn_sqrtf(v), c.fast_ibc, c.fast_eps);
        p = fmaf(m, __builtin_amdgcn_rcpf(d), p);
    } else {
        const float denom = div_by_const(sqrtf(v), c.bc2_sqrt, c.inv_bc2_sqrt) + c.eps;
        p = p + c.neg_step * (m / denom);
    }
}

// torch.optim.SGD single-tensor step (sgd.py _single_tensor_sgd; training.py:1324-1330):
//   grad = grad.add(param, alpha=wd)                  ATen add: fmadd(param, wd, grad)
//   buf  = grad.clone() (first step) | buf.mul_(momentum).add_(grad, alpha=1 - dampening)
//   grad = grad.add(buf, alpha=momentum) (nesterov) | buf ;  param.add_(grad, alpha=-lr)
// m is the momentum buffer; v aliases it (or, momentum == 0, both alias the parameter), so the
// callers' three stores all write the value that belongs at that address.
__device__ __forceinline__ void sgd_elem(float& p, float& m, float& v, float g, const AdamConsts& c) {
    if (c.wd != 0.f) g = fmaf(p, c.wd, g);
    if (c.sgd_mom != 0.f) {
        const float buf = c.sgd_first ? g : fmaf(g, c.sgd_damp1, m * c.sgd_mom);
        g = c.sgd_nesterov ? fmaf(buf, c.sgd_mom, g) : buf;
        p = fmaf(g, c.sgd_neg_lr, p);
        m = v = buf;
    } else {
        p = fmaf(g, c.sgd_neg_lr, p);
        m = v = p;
    }
}

__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, const AdamConsts& c) {
    if (c.sgd)
        sgd_elem(p, m, v, g, c);
    else if (c.decoupled)
        adam_elem_t<true>(p, m, v, g, c);
    else
        adam_elem_t<false>(p, m, v, g, c);
}
__device__ __forceinline__ void adam_elem_g0(float& p, float& m, float& v, const AdamConsts& c) {
    if (c.sgd) {
        sgd_elem(p, m, v, 0.f, c);
    } else if (c.fast_g0) {
        if (c.decoupled)
            adam_elem_t<true, true, true>(p, m, v, 0.f, c);
        else
            adam_elem_t<false, true, true>(p, m, v, 0.f, c);
    } else if (c.decoupled) {
        adam_elem_t<true, true>(p, m, v, 0.f, c);
    } else {
        adam_elem_t<false, true>(p, m, v, 0.f, c);
    }
}

// torch SparseAdam on one coalesced element (_functional.py:61-84).
__device__ __forceinline__ void sparse_adam_elem(float& p, float& m, float& v, float g, const SparseConsts& c) {
    const float om = m, ov = v;
    float um = (g - om) * c.w1;
    float uv = (g * g - ov) * c.w2;
    m = om + um;
    v = ov + uv;
    const float numer = um + om;
    const float denom = sqrtf(uv + ov) + c.eps;
    p = p + c.neg_step * (numer / denom);
}

}  // namespace

}  // namespace ttamm
