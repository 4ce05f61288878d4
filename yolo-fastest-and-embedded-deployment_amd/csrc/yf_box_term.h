// yf_box_term.h -- the IoU-family box term of ONE positive cell and its derivative with respect to the cell's four logits, in double
// (yolo_fastest_hip.h: yf_train_head_loss_box states the definition).  Plain C++ that compiles for the host as well, so that the
// derivative can be held to float64 autograd on the CPU; loss_cells_kernel<GRAD, true> (yf_loss_kernels.hip) is its only user.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define YF_BOX_HD __host__ __device__ __forceinline__
#else
#define YF_BOX_HD inline
#endif

namespace yf {

enum { BOX_REF = 0, BOX_GIOU = 1, BOX_DIOU = 2, BOX_CIOU = 3 };   // = YF_BOX_* of the header
constexpr double BOX_WH_CLAMP = 10.0;                             // = YF_BOX_WH_CLAMP
constexpr double BOX_EPS = 1e-7;

// d max(a, b) / da and d min(a, b) / da with torch's convention at a tie: one half each
YF_BOX_HD double box_dmax(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }
YF_BOX_HD double box_dmin(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }

// t[4]: the logits; (aw, ah): the anchor in feature-map units; (tx, ty, gw, gh): the target box.  Returns the value (GIoU, DIoU or
// CIoU of the predicted box against the target) and, if dt is not null, dt[c] = d value / d t[c].
// The derivative is taken in two steps.  First with respect to the predicted box's corners x1, x2, y1, y2 (gx1 .. gy2) and to its size
// where the size enters directly (gpw, gph: the area in the union, the aspect term of CIoU); then corners = centre -+ size / 2 and
// the centre = sigmoid(t), the size = exp(clamp(t)) * anchor.  The clamp's derivative is torch's: 1 on [-10, 10] inclusive, 0 outside.
YF_BOX_HD double box_term(int kind, const double t[4], double aw, double ah, double tx, double ty, double gw, double gh, double* dt)
{
    const double px = 1.0 / (1.0 + exp(-t[0])), py = 1.0 / (1.0 + exp(-t[1]));
    const double pw = exp(fmin(fmax(t[2], -BOX_WH_CLAMP), BOX_WH_CLAMP)) * aw, ph = exp(fmin(fmax(t[3], -BOX_WH_CLAMP), BOX_WH_CLAMP)) * ah;
    const double ax1 = px - pw * 0.5, ax2 = px + pw * 0.5, ay1 = py - ph * 0.5, ay2 = py + ph * 0.5;   // predicted box
    const double bx1 = tx - gw * 0.5, bx2 = tx + gw * 0.5, by1 = ty - gh * 0.5, by2 = ty + gh * 0.5;   // target box
    const double ex = fmin(ax2, bx2) - fmax(ax1, bx1), ey = fmin(ay2, by2) - fmax(ay1, by1);
    const double ix = fmax(ex, 0.0), iy = fmax(ey, 0.0);
    const double inter = ix * iy;
    const double uni = pw * ph + gw * gh - inter + BOX_EPS;
    const double iou = inter / uni;
    const double cw = fmax(ax2, bx2) - fmin(ax1, bx1), ch = fmax(ay2, by2) - fmin(ay1, by1);
    // d inter / d corner (clamp(min = 0) passes the gradient at 0, like torch)
    const double sx = ex >= 0.0 ? iy : 0.0, sy = ey >= 0.0 ? ix : 0.0;
    const double ix1 = -sx * box_dmax(ax1, bx1), ix2 = sx * box_dmin(ax2, bx2), iy1 = -sy * box_dmax(ay1, by1), iy2 = sy * box_dmin(ay2, by2);
    // d cw / d x1, x2 and d ch / d y1, y2
    const double cx1 = -box_dmin(ax1, bx1), cx2 = box_dmax(ax2, bx2), cy1 = -box_dmin(ay1, by1), cy2 = box_dmax(ay2, by2);
    // iou = inter / uni, uni = pw ph + gw gh - inter + eps:  d iou = ki d inter + ka d(pw ph)
    const double ki = (uni + inter) / (uni * uni), ka = -inter / (uni * uni);
    double gx1 = ki * ix1, gx2 = ki * ix2, gy1 = ki * iy1, gy2 = ki * iy2, gpw = ka * ph, gph = ka * pw;
    double value;
    if (kind == BOX_GIOU) {
        // giou = iou - 1 + uni / c, c = cw ch + eps:  d = d iou + (d(pw ph) - d inter) / c - uni / c^2 (ch d cw + cw d ch)
        const double c = cw * ch + BOX_EPS, kc = -uni / (c * c);
        value = iou - (c - uni) / c;
        gx1 += -ix1 / c + kc * ch * cx1; gx2 += -ix2 / c + kc * ch * cx2;
        gy1 += -iy1 / c + kc * cw * cy1; gy2 += -iy2 / c + kc * cw * cy2;
        gpw += ph / c; gph += pw / c;
    } else {
        // diou = iou - rho2 / c2, c2 = cw^2 + ch^2 + eps, rho2 = (dx^2 + dy^2) / 4 with dx = bx1 + bx2 - x1 - x2
        const double c2 = cw * cw + ch * ch + BOX_EPS;
        const double dx = bx1 + bx2 - ax1 - ax2, dy = by1 + by2 - ay1 - ay2;
        const double rho2 = (dx * dx + dy * dy) * 0.25;
        const double kr = 0.5 / c2, kc = rho2 / (c2 * c2) * 2.0;       // - d rho2 / c2 = dx / (2 c2) per corner;  + rho2 / c2^2 d c2
        value = iou - rho2 / c2;
        gx1 += kr * dx + kc * cw * cx1; gx2 += kr * dx + kc * cw * cx2;
        gy1 += kr * dy + kc * ch * cy1; gy2 += kr * dy + kc * ch * cy2;
        if (kind == BOX_CIOU) {
            // v = 4 / pi^2 (atan(gw / (gh + eps)) - atan(pw / (ph + eps)))^2, alpha = v / (v - iou + 1 + eps) held constant
            const double k4 = 4.0 / (M_PI * M_PI), q = pw / (ph + BOX_EPS), da = atan(gw / (gh + BOX_EPS)) - atan(q);
            const double v = k4 * da * da, alpha = v / (v - iou + 1.0 + BOX_EPS);
            const double dvq = -k4 * 2.0 * da / (1.0 + q * q);         // d v / d q
            value -= v * alpha;
            gpw -= alpha * dvq / (ph + BOX_EPS);
            gph += alpha * dvq * q / (ph + BOX_EPS);
        }
    }
    if (dt) {
        const double dpw = pw * (fabs(t[2]) <= BOX_WH_CLAMP ? 1.0 : 0.0), dph = ph * (fabs(t[3]) <= BOX_WH_CLAMP ? 1.0 : 0.0);
        dt[0] = (gx1 + gx2) * (1.0 - px) * px;
        dt[1] = (gy1 + gy2) * (1.0 - py) * py;
        dt[2] = ((gx2 - gx1) * 0.5 + gpw) * dpw;
        dt[3] = ((gy2 - gy1) * 0.5 + gph) * dph;
    }
    return value;
}

}  // namespace yf
