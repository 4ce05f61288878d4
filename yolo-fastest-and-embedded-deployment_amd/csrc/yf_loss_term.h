// yf_loss_term.h -- ONE binary-cross-entropy element of the objectness / class loss under yolov5's loss options (positive weight, soft
// target, focal wrap) and its derivative with respect to the probability, in double (yolo_fastest_hip.h: yf_train_head_loss_hyp states
// the definition).  Plain C++ that compiles for the host as well, like yf_box_term.h, so that the derivative can be held to float64
// autograd on the CPU; loss_cells_kernel<GRAD, BOX, true> (yf_loss_kernels.hip) is its only user.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define YF_TERM_HD __host__ __device__ __forceinline__
#else
#define YF_TERM_HD inline
#endif

namespace yf {

// p: the (float32-rounded) sigmoid, t: the target in [0, 1], w: the positive weight.
//   base = -(w t max(log p, -100) + (1 - t) max(log(1 - p), -100))          torch's BCELoss element with BCEWithLogits' pos_weight
//   d base / d p = (-w t (1 - p) + (1 - t) p) / max((1 - p) p, 1e-12)       torch's BCELoss backward, its clamp included
// gamma > 0 wraps it like yolov5's FocalLoss (gamma == 0: nothing wraps it and alpha is not read):
//   p_t = t p + (1 - t)(1 - p)    af = t alpha + (1 - t)(1 - alpha)    elem = base af (1 - p_t)^gamma
//   d (1 - p_t)^gamma / d p = gamma (1 - p_t)^(gamma - 1) (1 - 2 t)         the modulating factor is NOT a constant in the backward
// gamma >= 1 keeps (1 - p_t)^(gamma - 1) finite at p_t = 1 (pow(0, 0) = 1); 0 < gamma < 1 is refused by the entry.
// Returns the element and, if dp is not null, *dp = d elem / d p (times (1 - p) p for the logit, which the caller applies).
YF_TERM_HD double loss_elem(double p, double t, double w, double gamma, double alpha, double* dp)
{
    const double base = -(w * t * fmax(log(p), -100.0) + (1.0 - t) * fmax(log(1.0 - p), -100.0));
    const double dbase = (-w * t * (1.0 - p) + (1.0 - t) * p) / fmax((1.0 - p) * p, 1e-12);
    if (!(gamma > 0.0)) {
        if (dp) *dp = dbase;
        return base;
    }
    const double q = fmax(1.0 - (t * p + (1.0 - t) * (1.0 - p)), 0.0);       // 1 - p_t (the max only keeps a rounding below 0 out of pow)
    const double af = t * alpha + (1.0 - t) * (1.0 - alpha);
    const double q1 = pow(q, gamma - 1.0), mod = q1 * q;
    if (dp) *dp = af * (dbase * mod + base * (gamma * q1 * (1.0 - 2.0 * t)));
    return base * af * mod;
}

}  // namespace yf
