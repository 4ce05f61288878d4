// yf_loss_kernels.hip -- the loss end of the reference's training step (first slice):
//   YOLOLossV3.forward(input, targets)   src/model_training/loss/yolo_loss.py:48-97   (loss terms)
//   YOLOLossV3.get_target                src/model_training/loss/yolo_loss.py:144-196 (targets -> dense masks)
// plus d(total loss)/d(input), what `loss.backward()` (src/model_training/train.py:131) hands to the head tensors.
//
// Three small launches per head (HBM-bound, a few MB): init of the dense target arrays, one thread per image walking its
// targets IN ORDER (the reference's loop has sequential semantics: a later target overwrites an earlier one in the same cell),
// and one pass over all cells that accumulates the seven sums in double (block reduction + one atomicAdd per block) and
// writes the gradient.  The backward of the layers themselves is not part of this slice.
//
// yf_train_head_loss_box (opt-in) regresses the box as ONE IoU-family term per positive cell in place of the reference's four
// (yf_box_term.h): two more target planes and loss_cells_kernel<GRAD, true>, the same five launches.
//
// yf_train_head_loss_hyp (opt-in) adds yolov5's objectness / class options to either: loss_cells_kernel<GRAD, BOX, true> evaluates the
// BCE elements a non-neutral option touches through yf_loss_term.h, loss_final_kernel applies the two gains; five launches again.
// One launcher (launch_train_loss) and one loss_final_kernel serve all three entries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "yf_box_term.h"
#include "yf_loss_term.h"
#include "yf_kernels.h"

namespace yf {

// dense target arrays, per (n, anchor, row, col): mask, noobj, tx, ty, tw, th, tcls0..nc-1   (6 + num_classes planes)
// yf_train_head_loss_box: two more behind the class planes, gw and gh of the target that wrote tx (feature-map units)
enum { LT_MASK = 0, LT_NOOBJ, LT_TX, LT_TY, LT_TW, LT_TH, LT_C0 };
enum { LOSS_MAX_ANCHORS = 8 };
struct LossAnchors { float w[LOSS_MAX_ANCHORS], h[LOSS_MAX_ANCHORS]; };

__global__ void loss_init_kernel(float* __restrict__ dense, long E, int planes, double* __restrict__ acc)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < 16 && blockIdx.x == 0) acc[e] = 0.0;
    if (e >= E) return;
    for (int p = 0; p < planes; ++p) dense[p * E + e] = p == LT_NOOBJ ? 1.f : 0.f;
}

// yolo_loss.py:156-194 for image n.  anc: the three (w, h) anchors in feature-map units as float32 (torch turns the Python-double
// scaled anchors into float32 for both the IoU and the division).  acc[8] counts the targets the reference cannot index: a cell
// outside the map, or a class outside 0 .. nc-1 (:195 raises IndexError).  Such a target is skipped whole.  (A NEGATIVE index wraps
// round in the reference; that is not reproduced: it is counted like any other index outside the range.)
__global__ void loss_targets_kernel(const float* __restrict__ targets, int T, float* __restrict__ dense, long E, int N, int fh, int fw,
                                    LossAnchors anc, int na, int nc, float ignore_thres, double* __restrict__ acc, int size_planes)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* aw = anc.w;
    const float* ah = anc.h;
    for (int t = 0; t < T; ++t) {
        const float* g = targets + ((long)n * T + t) * 6;
        if (g[5] < 1.f) break;                                         // :158 the marker ends the list
        const float gx = g[0] * (float)fw, gy = g[1] * (float)fh, gw = g[2] * (float)fw, gh = g[3] * (float)fh;   // :161-164
        if (gw <= 0.f || gh <= 0.f) continue;                          // :166
        const int gi = (int)gx, gj = (int)gy;                          // :170-171 int() truncates
        const int c = (int)g[4];                                       // :195 int() truncates
        if (gi < 0 || gi >= fw || gj < 0 || gj >= fh || c < 0 || c >= nc) { atomicAdd(&acc[8], 1.0); continue; }
        float iou[LOSS_MAX_ANCHORS];
        int best = 0;
        for (int a = 0; a < na; ++a) {                                 // bbox_iou([0,0,gw,gh], [0,0,aw,ah]), +1 convention (general.py:29-52)
            const float iw = fmaxf(fminf(gw, aw[a]) - 0.f + 1.f, 0.f), ih = fmaxf(fminf(gh, ah[a]) - 0.f + 1.f, 0.f);
            const float inter = iw * ih;
            const float b1 = (gw - 0.f + 1.f) * (gh - 0.f + 1.f), b2 = (aw[a] - 0.f + 1.f) * (ah[a] - 0.f + 1.f);
            iou[a] = inter / (b1 + b2 - inter + 1e-16f);
            if (iou[a] > iou[best]) best = a;                          // np.argmax: first maximum
        }
        const long cell = (long)gj * fw + gi;
        for (int a = 0; a < na; ++a)
            if (iou[a] > ignore_thres) dense[LT_NOOBJ * E + ((long)n * na + a) * fh * fw + cell] = 0.f;   // :181
        const long e = ((long)n * na + best) * fh * fw + cell;
        dense[LT_MASK * E + e] = 1.f;                                  // :184
        dense[LT_TX * E + e] = gx - (float)gi;                         // :187-188
        dense[LT_TY * E + e] = gy - (float)gj;
        dense[LT_TW * E + e] = (float)log((double)(gw / aw[best] + 1e-16f));   // :190-191 math.log of the float32 quotient, in double
        dense[LT_TH * E + e] = (float)log((double)(gh / ah[best] + 1e-16f));
        dense[(LT_C0 + c) * E + e] = 1.f;                              // :195 one-hot (accumulates over targets sharing the cell)
        if (size_planes) {                                             // the box loss's target size: the last target's, like tx
            dense[(LT_C0 + nc) * E + e] = gw;
            dense[(LT_C0 + nc + 1) * E + e] = gh;
        }
    }
}

// torch.nn.BCELoss element: -(t * max(log p, -100) + (1 - t) * max(log(1 - p), -100))
__device__ __forceinline__ float bce(float p, float t) { return -(t * fmaxf(logf(p), -100.f) + (1.f - t) * fmaxf(logf(1.f - p), -100.f)); }
// its derivative with respect to p: (p - t) / max((1 - p) p, 1e-12)
__device__ __forceinline__ float dbce(float p, float t) { return (p - t) / fmaxf((1.f - p) * p, 1e-12f); }
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
// d(conf) / d(confidence logit) and d(cls) / d(class logit) of the reference's terms in float32: inv = 1 / E, m and nm the two masks
__device__ __forceinline__ float conf_grad(float pc, float m, float nm, float inv)
{
    return inv * (dbce(pc * m, m) * m + 0.5f * dbce(pc * nm, 0.f) * nm) * (1.f - pc) * pc;
}
__device__ __forceinline__ float cls_grad(float pk, float tk, int nc, float npos) { return dbce(pk, tk) * (1.f - pk) * pk / ((float)nc * npos); }

// what loss_cells_kernel<GRAD, true> needs on top: the anchors the targets were matched with, which IoU-family term, and its weight
struct LossBox { LossAnchors anc; int na, kind; double lambda; };
// what loss_cells_kernel<GRAD, BOX, true> needs on top of that: the options of yf_train_head_loss_hyp by value.  cp, cn: the smoothed
// class targets.  conf_plain / cls_plain: no option touches that term's elements (only its gain may differ from 1), which then stay the
// float32 arithmetic of the other instantiations, bit for bit; otherwise they are loss_elem's, in double on the float32 sigmoid.
struct LossHyp { double obj_pw, cls_pw, gamma, alpha, obj_iou, lambda_conf, lambda_cls; float cp, cn; int conf_plain, cls_plain; };
struct LossBoxHyp : LossBox { LossHyp hyp; };
template <bool HYP> struct LossArgs { using type = LossBox; };
template <> struct LossArgs<true> { using type = LossBoxHyp; };

// acc: [0] sum bce x, [1] y, [2] sum (w)^2, [3] h, [4] conf obj, [5] conf noobj, [6] cls, [7] n_pos
// BOX: [0] sum over the positive cells of 1 - value (yf_box_term.h, evaluated in double per positive cell: a float32 evaluation
// cancels in GIoU's enclosing-area term for a clamped, huge box), [1..3] zero; channels 0..3 of the gradient are lambda / E times
// its derivative, rounded to float32 once at the store, an exact 0 at every other cell.  Channels 4.. as without BOX.
// HYP: [4], [5], [6] are sums of loss_elem's elements where an option touches them (the objectness target of a positive cell is then
// t_obj, the class targets cp / cn); channel 4 of the gradient carries lambda_conf, channels 5.. lambda_cls.
template <bool GRAD, bool BOX, bool HYP = false>
__global__ void __launch_bounds__(256) loss_cells_kernel(const float* __restrict__ head, const float* __restrict__ dense, long E, int fh, int fw,
                                                         int nc, double* __restrict__ acc, float* __restrict__ grad, typename LossArgs<HYP>::type box)
{
    const int attrs = 5 + nc;
    __shared__ double red[8][4];
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (e < E) {
        const long hw = (long)fh * fw;
        const long na = e / hw, cell = e - na * hw;          // na = n * num_anchors + anchor
        const float* t = head + na * attrs * hw + cell;      // [N, A*(5+C), fh, fw]: channel c of this anchor at t[c * hw]
        const float m = dense[LT_MASK * E + e], nm = dense[LT_NOOBJ * E + e];
        const float px = sigm(t[0]), py = sigm(t[hw]), w = t[2 * hw], h = t[3 * hw], pc = sigm(t[4 * hw]);
        const float tx = dense[LT_TX * E + e], ty = dense[LT_TY * E + e], tw = dense[LT_TW * E + e], th = dense[LT_TH * E + e];
        const float dw = w * m - tw * m, dh = h * m - th * m;
        double dbox[4] = {0, 0, 0, 0};                       // BOX: d value / d logit of this cell
        [[maybe_unused]] float tobj = 1.f;                   // HYP: the objectness target of a positive cell
        [[maybe_unused]] double dobj = 0, dnoobj = 0;        // HYP: d element / d pc of the two confidence elements
        if constexpr (BOX) {
            if (m == 1.f) {
                const int a = (int)(na % box.na);
                const double tl[4] = {(double)t[0], (double)t[hw], (double)w, (double)h};
                const double value = box_term(box.kind, tl, (double)box.anc.w[a], (double)box.anc.h[a], (double)tx, (double)ty,
                                              (double)dense[(LT_C0 + nc) * E + e], (double)dense[(LT_C0 + nc + 1) * E + e], GRAD ? dbox : nullptr);
                s[0] = 1.0 - value;
                if constexpr (HYP)                           // a constant in the backward (yolov5's iou.detach().clamp(0))
                    if (box.hyp.obj_iou > 0.0) tobj = (float)((1.0 - box.hyp.obj_iou) + box.hyp.obj_iou * fmin(fmax(value, 0.0), 1.0));
            }
        } else {
            s[0] = bce(px * m, tx * m);                      // yolo_loss.py:78-79
            s[1] = bce(py * m, ty * m);
            s[2] = dw * dw;                                  // :80-81
            s[3] = dh * dh;
        }
        bool conf_plain = true, cls_plain = true;
        if constexpr (HYP) { conf_plain = box.hyp.conf_plain; cls_plain = box.hyp.cls_plain; }
        if (conf_plain) {
            s[4] = bce(pc * m, m);                           // :84
            s[5] = bce(pc * nm, nm * 0.f);
        } else if constexpr (HYP) {                          // both masks are 0 or 1; a masked-out element is an exact 0, as above
            if (m == 1.f) s[4] = loss_elem((double)pc, (double)tobj, box.hyp.obj_pw, box.hyp.gamma, box.hyp.alpha, GRAD ? &dobj : nullptr);
            if (nm == 1.f) s[5] = loss_elem((double)pc, 0.0, 1.0, box.hyp.gamma, box.hyp.alpha, GRAD ? &dnoobj : nullptr);
        }
        if (m == 1.f) {                                      // :87 pred_cls[mask == 1]
            if (cls_plain) {
                for (int k = 0; k < nc; ++k) s[6] += bce(sigm(t[(5 + k) * hw]), dense[(LT_C0 + k) * E + e]);
            } else if constexpr (HYP) {
                for (int k = 0; k < nc; ++k)
                    s[6] += loss_elem((double)sigm(t[(5 + k) * hw]), (double)(dense[(LT_C0 + k) * E + e] == 1.f ? box.hyp.cp : box.hyp.cn),
                                      box.hyp.cls_pw, box.hyp.gamma, box.hyp.alpha, nullptr);
            }
            s[7] = 1.0;
        }
        if constexpr (GRAD) {
            // acc[7] already holds n_pos (the forward pass ran first); d(total)/d(logit), total = 2.5 (x + y + w + h) + conf + cls
            const float inv = 1.f / (float)E, npos = (float)acc[7];
            float* g = grad + na * attrs * hw + cell;
            if constexpr (BOX) {
                const double k = -box.lambda / (double)E;    // total = lambda * (1 / E) sum (1 - value) + conf + cls
                for (int c = 0; c < 4; ++c) g[c * hw] = m == 1.f ? (float)(k * dbox[c]) : 0.f;
            } else {
                g[0] = 2.5f * inv * dbce(px * m, tx * m) * m * (1.f - px) * px;
                g[hw] = 2.5f * inv * dbce(py * m, ty * m) * m * (1.f - py) * py;
                g[2 * hw] = 2.5f * inv * 2.f * dw * m;
                g[3 * hw] = 2.5f * inv * 2.f * dh * m;
            }
            if constexpr (!HYP) {
                g[4 * hw] = conf_grad(pc, m, nm, inv);
                for (int k = 0; k < nc; ++k)
                    g[(5 + k) * hw] = m == 1.f ? cls_grad(sigm(t[(5 + k) * hw]), dense[(LT_C0 + k) * E + e], nc, npos) : 0.f;
            } else {
                // total = [box part] + lambda_conf conf + lambda_cls cls.  A plain term: the float32 value above times the float32 gain (a
                // gain of 2 doubles its bits); otherwise everything in double, rounded to float32 once at the store
                const LossHyp& hp = box.hyp;
                if (conf_plain)
                    g[4 * hw] = (float)hp.lambda_conf * conf_grad(pc, m, nm, inv);
                else
                    g[4 * hw] = (float)(hp.lambda_conf / (double)E * (dobj + 0.5 * dnoobj) * (1.0 - (double)pc) * (double)pc);
                for (int k = 0; k < nc; ++k) {
                    float gk = 0.f;
                    if (m == 1.f) {
                        const float pk = sigm(t[(5 + k) * hw]), tk = dense[(LT_C0 + k) * E + e];
                        if (cls_plain) {
                            gk = (float)hp.lambda_cls * cls_grad(pk, tk, nc, npos);
                        } else {
                            double d;
                            loss_elem((double)pk, (double)(tk == 1.f ? hp.cp : hp.cn), hp.cls_pw, hp.gamma, hp.alpha, &d);
                            gk = (float)(hp.lambda_cls * d * (1.0 - (double)pk) * (double)pk / ((double)nc * acc[7]));
                        }
                    }
                    g[(5 + k) * hw] = gk;
                }
            }
            return;
        }
    }
    if constexpr (!GRAD) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double v = s[k];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
            if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
        }
        __syncthreads();
        if (threadIdx.x < 8) atomicAdd(&acc[threadIdx.x], red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
    }
}

// losses[0..7] = total, x, y, w, h, conf, cls (float32, combined like yolo_loss.py:90-92), targets skipped (cell outside the map or class
// outside 0 .. nc-1).  box: total, box, 0, 0, 0, conf, cls, targets skipped; total = lambda * box + conf + cls in float32, left to right.
// lambda_conf / lambda_cls: the gains of yf_train_head_loss_hyp on conf and cls in the total (1.0f elsewhere: x * 1.0f is x); [5] and [6]
// stay unweighted
__global__ void loss_final_kernel(const double* __restrict__ acc, long E, int nc, int box, float lambda, float lambda_conf, float lambda_cls,
                                  float* __restrict__ losses)
{
    const float lx = (float)(acc[0] / (double)E), ly = (float)(acc[1] / (double)E), lw = (float)(acc[2] / (double)E), lh = (float)(acc[3] / (double)E);
    const float lconf = (float)(acc[4] / (double)E) + 0.5f * (float)(acc[5] / (double)E);
    const float lcls = (float)(acc[6] / ((double)nc * acc[7]));     // no positive cell: 0 / 0 = nan, like the mean of an empty tensor
    if (box) {
        losses[0] = lambda * lx + lconf * lambda_conf + lcls * lambda_cls;
        losses[1] = lx; losses[2] = 0.f; losses[3] = 0.f; losses[4] = 0.f;
    } else {
        losses[0] = lx * 2.5f + ly * 2.5f + lw * 2.5f + lh * 2.5f + lconf * lambda_conf + lcls * lambda_cls;
        losses[1] = lx; losses[2] = ly; losses[3] = lw; losses[4] = lh;
    }
    losses[5] = lconf; losses[6] = lcls;
    losses[7] = (float)acc[8];
}

size_t train_loss_workspace_bytes(int N, int fh, int fw, int na, int nc, int size_planes)
{
    return ((size_t)(LT_C0 + nc + 2 * size_planes) * N * na * fh * fw) * sizeof(float) + 16 * sizeof(double) + 64;
}

// the forward pass over all cells, then (grad) the backward one, of one of the four (BOX, HYP) pairs
template <bool BOX, bool HYP>
static void launch_cells(const float* head, const float* dense, long E, int fh, int fw, int nc, double* acc, float* grad, const LossBoxHyp& lb,
                         hipStream_t s)
{
    const typename LossArgs<HYP>::type& arg = lb;
    const unsigned nb = (unsigned)((E + 255) / 256);
    hipLaunchKernelGGL((loss_cells_kernel<false, BOX, HYP>), dim3(nb), dim3(256), 0, s, head, dense, E, fh, fw, nc, acc, (float*)nullptr, arg);
    if (grad) hipLaunchKernelGGL((loss_cells_kernel<true, BOX, HYP>), dim3(nb), dim3(256), 0, s, head, dense, E, fh, fw, nc, acc, grad, arg);
}

// spec.hyp: opt[8] = obj_pw, cls_pw, label_smoothing, fl_gamma, fl_alpha, obj_iou, lambda_conf, lambda_cls (validated by the entry).  With
// every option neutral (or no options) the plain instantiations run: the same kernels as without options, hence the same bits.
void launch_train_loss(const float* head, int N, int fh, int fw, const float* anc, int na, int nc, const float* targets, int T, float ignore_thres,
                       void* work, float* losses, float* grad, const LossSpec& spec, hipStream_t s)
{
    const long E = (long)N * na * fh * fw;
    const bool box = spec.box_kind > 0;
    const int sizes = spec.box_kind >= 0;
    LossBoxHyp lb{};
    for (int a = 0; a < na && a < LOSS_MAX_ANCHORS; ++a) { lb.anc.w[a] = anc[2 * a]; lb.anc.h[a] = anc[2 * a + 1]; }
    lb.na = na; lb.kind = spec.box_kind; lb.lambda = spec.lambda_box;
    bool plain = true;
    float lambda_conf = 1.0f, lambda_cls = 1.0f;
    if (const double* opt = spec.hyp) {
        const bool focal = opt[3] > 0.0;
        LossHyp& hp = lb.hyp;
        hp.obj_pw = opt[0]; hp.cls_pw = opt[1]; hp.gamma = opt[3]; hp.alpha = opt[4]; hp.obj_iou = opt[5]; hp.lambda_conf = opt[6]; hp.lambda_cls = opt[7];
        hp.cp = (float)(1.0 - 0.5 * opt[2]); hp.cn = (float)(0.5 * opt[2]);
        hp.conf_plain = opt[0] == 1.0 && !focal && opt[5] == 0.0;
        hp.cls_plain = opt[1] == 1.0 && !focal && opt[2] == 0.0;
        plain = hp.conf_plain && hp.cls_plain && opt[6] == 1.0 && opt[7] == 1.0;
        lambda_conf = (float)opt[6]; lambda_cls = (float)opt[7];
    }
    double* acc = reinterpret_cast<double*>(work);                       // 16 doubles first (8-byte aligned), the dense planes behind
    float* dense = reinterpret_cast<float*>(static_cast<char*>(work) + 16 * sizeof(double));
    hipLaunchKernelGGL(loss_init_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, dense, E, LT_C0 + nc + 2 * sizes, acc);
    hipLaunchKernelGGL(loss_targets_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, targets, T, dense, E, N, fh, fw, lb.anc, na, nc,
                       ignore_thres, acc, sizes);
    if (plain) (box ? launch_cells<true, false> : launch_cells<false, false>)(head, dense, E, fh, fw, nc, acc, grad, lb, s);
    else       (box ? launch_cells<true, true> : launch_cells<false, true>)(head, dense, E, fh, fw, nc, acc, grad, lb, s);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(1), 0, s, acc, E, nc, (int)box, (float)spec.lambda_box, lambda_conf, lambda_cls, losses);
}

}  // namespace yf
